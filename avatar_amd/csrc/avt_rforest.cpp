// avt_rforest.cpp — host side of the forest of several trees (include/avt_rforest.h): validation of the members against each
// other, the packed device image (one node array with rebased links, one leaf table) and the score.  Image staging and the
// resident forms are the labelling handle's (avt_label.cpp), as for one tree.
#include "avt_rforest.h"

#include <algorithm>
#include <string>

#include "avt_internal.h"
#include "avt_rtree_train.h"

namespace {

const AvtLabelNames kForest = {"rforest", "avt_rforest", "forest"};
const char* const kHostOnly = "rforest: created host-only (device < 0): inference needs a GPU";      // the score's own checks
const int kMaxImages = 65535;     // blockIdx.z is the image

// the launches behind the shared image side (avt_label.cpp)
int launch_boxes(AvtLabelHandle* h, const float* d_depth, const int* d_boxes, int box_stride, int n_images, int rows, int cols, int interval, int fill) {
    return avt_rforest_launch_predict(static_cast<avt_rforest*>(h), d_depth, d_boxes, box_stride, n_images, rows, cols, interval, 0, 0, 0, 0, fill);
}
int launch_dist(AvtLabelHandle* h, int rows, int cols, float* d_out) { return avt_rforest_launch_predict_dist(static_cast<avt_rforest*>(h), rows, cols, d_out); }

// every tree's nodes behind each other, links rebased; a leaf's rnode is its row in the forest's one table
int pack(avt_rforest* rf, const avt_rtree* const* trees) {
    size_t n_total = 0, l_total = 0;
    for (int t = 0; t < rf->n_trees; ++t) { n_total += trees[t]->links.size() / 3; l_total += trees[t]->leaf_best.size(); }
    if (n_total >= (1u << 30) || l_total * (size_t)rf->num_parts >= (1u << 30)) { avt_set_error("avt_rforest_create: the forest is too large"); return 1; }
    rf->nodes.reserve(n_total);
    rf->leaf.reserve(l_total * rf->num_parts);
    for (int t = 0; t < rf->n_trees; ++t) {
        const avt_rtree* rt = trees[t];
        const int n = (int)(rt->links.size() / 3), node0 = (int)rf->nodes.size(), leaf0 = (int)(rf->leaf.size() / rf->num_parts);
        rf->roots.push_back(node0);
        for (int i = 0; i < n; ++i) {
            const float* f = &rt->feature[5 * (size_t)i];
            const int leaf = rt->links[3 * i + 2];
            rf->nodes.push_back(RtNodeDev{f[0], f[1], f[2], f[3], f[4], leaf < 0 ? node0 + rt->links[3 * i] : (int)rt->leaf_best[leaf],
                                          leaf < 0 ? node0 + rt->links[3 * i + 1] : leaf0 + leaf, leaf < 0 ? 0 : 1});
        }
        rf->leaf.insert(rf->leaf.end(), rt->leaf_data.begin(), rt->leaf_data.end());
    }
    return 0;
}

int upload_forest(avt_rforest* rf) {
    if (rf->device < 0) return 0;
    AVT_HIP(hipSetDevice(rf->device));
    AVT_HIP(hipStreamCreateWithFlags(&rf->stream, hipStreamNonBlocking));
    if (rf->d_nodes.reserve(rf->nodes.size()) || rf->d_roots.reserve(rf->roots.size()) || rf->d_leaf.reserve(std::max<size_t>(1, rf->leaf.size()))) return 1;
    AVT_HIP(hipMemcpyAsync(rf->d_nodes, rf->nodes.data(), sizeof(RtNodeDev) * rf->nodes.size(), hipMemcpyHostToDevice, rf->stream));
    AVT_HIP(hipMemcpyAsync(rf->d_roots, rf->roots.data(), sizeof(int) * rf->roots.size(), hipMemcpyHostToDevice, rf->stream));
    AVT_HIP(hipMemcpyAsync(rf->d_leaf, rf->leaf.data(), sizeof(float) * rf->leaf.size(), hipMemcpyHostToDevice, rf->stream));
    AVT_HIP(hipStreamSynchronize(rf->stream));     // the legacy stream is never used (a host thread may be capturing)
    return 0;
}

int create_impl(const avt_rtree* const* trees, int n_trees, int device, avt_rforest** out) {
    if (!trees || !out) { avt_set_error("avt_rforest_create: null argument"); return 1; }
    if (n_trees < 1 || n_trees > AVT_RFOREST_MAX_TREES) {
        avt_set_error("avt_rforest_create: " + std::to_string(n_trees) + " trees: a forest has 1 to " + std::to_string(AVT_RFOREST_MAX_TREES));
        return 1;
    }
    for (int t = 0; t < n_trees; ++t) {
        if (!trees[t]) { avt_set_error("avt_rforest_create: tree " + std::to_string(t) + " is null"); return 1; }
        const std::string who = "avt_rforest_create: tree " + std::to_string(t);
        if (trees[t]->num_parts != trees[0]->num_parts) {
            avt_set_error(who + " has num_parts " + std::to_string(trees[t]->num_parts) + ", tree 0 has " + std::to_string(trees[0]->num_parts));
            return 1;
        }
        if (trees[t]->part_map != trees[0]->part_map) { avt_set_error(who + " has another part map than tree 0"); return 1; }
        if (trees[t]->part_map_type != trees[0]->part_map_type) { avt_set_error(who + " has another part-map type than tree 0"); return 1; }
    }
    avt_rforest* rf = new avt_rforest();
    rf->device = device;
    rf->n_trees = n_trees;
    rf->num_parts = trees[0]->num_parts;
    rf->part_map = trees[0]->part_map;
    rf->part_map_type = trees[0]->part_map_type;
    if (pack(rf, trees) || upload_forest(rf)) { avt_rforest_destroy(rf); return 1; }
    *out = rf;
    return 0;
}

int predict_best_impl(avt_rforest* rf, const float* depth, int rows, int cols, int interval, int tlx, int tly, int brx, int bry, int fill,
                      unsigned char* labels_out) {
    if (!rf || !depth || !labels_out) { avt_set_error("avt_rforest_predict_best: null argument"); return 1; }
    if (avt_label_roi_ok(kForest, rows, cols, interval, tlx, tly, brx, bry)) return 1;
    if (avt_label_images_upload(rf, kForest, kMaxImages, 1, rows, cols, depth)) return 1;
    if (avt_rforest_launch_predict(rf, rf->d_depth, nullptr, 0, 1, rows, cols, interval, tlx, tly, brx, bry, fill)) {
        avt_set_error("rforest: kernel launch failed");
        return 1;
    }
    return avt_label_labels_download(rf, kForest, 0, labels_out);
}

// ---- the score (include/avt_rforest.h): a call counts into the scratch matrix and is committed only when no label was refused
int score_begin(avt_rforest* rf) {
    const size_t cells = (size_t)(rf->num_parts + 1) * (rf->num_parts + 1);
    if (rf->d_score.reserve(cells) || rf->d_score_bad.reserve(1)) return 1;
    AVT_HIP(hipMemsetAsync(rf->d_score, 0, cells * sizeof(unsigned long long), rf->stream));
    AVT_HIP(hipMemsetAsync(rf->d_score_bad, 0, sizeof(int), rf->stream));
    return 0;
}

// waits for the call's kernels (also the contract of avt_renderer_images_for), then adds the scratch matrix to the totals
int score_commit(avt_rforest* rf, const char* who, int n_images, int rows, int cols, int stride) {
    const size_t cells = (size_t)(rf->num_parts + 1) * (rf->num_parts + 1);
    std::vector<unsigned long long> add(cells);
    int bad = 0;
    AVT_HIP(hipMemcpyAsync(add.data(), rf->d_score, cells * sizeof(unsigned long long), hipMemcpyDeviceToHost, rf->stream));
    AVT_HIP(hipMemcpyAsync(&bad, rf->d_score_bad, sizeof(int), hipMemcpyDeviceToHost, rf->stream));
    AVT_HIP(hipStreamSynchronize(rf->stream));
    if (bad) {
        avt_set_error(std::string(who) + ": a part-mask label is >= num_parts (" + std::to_string(rf->num_parts) + ") and not 255; the call's counts were dropped");
        return 1;
    }
    if (rf->score_conf.empty()) rf->score_conf.assign(cells, 0);
    for (size_t i = 0; i < cells; ++i) rf->score_conf[i] += (long long)add[i];
    rf->score_images += n_images;
    rf->score_pixels += (long long)n_images * ((rows - 1) / stride + 1) * ((cols - 1) / stride + 1);
    return 0;
}

int score_images_impl(avt_rforest* rf, int n, int rows, int cols, const float* depth, const unsigned char* mask, int stride) {
    const char* who = "avt_rforest_score_images";
    if (!rf || !depth || !mask) { avt_set_error(std::string(who) + ": null argument"); return 1; }
    if (n < 1 || rows < 1 || cols < 1 || stride < 1 || rows >= 32768 || cols >= 32768) {
        avt_set_error(std::string(who) + ": needs n_images >= 1, stride >= 1 and images of 1 to 32767 rows and columns");
        return 1;
    }
    if (rf->device < 0) { avt_set_error(kHostOnly); return 1; }
    AVT_HIP(hipSetDevice(rf->device));
    // staged in buffers of this call, in bounded batches: the resident images and labels are not touched
    const size_t npix = (size_t)rows * cols;
    const int batch = (int)std::max<size_t>(1, std::min<size_t>(n, ((size_t)256 << 20) / (npix * 5)));
    DevBuf<float> d_depth;
    DevBuf<unsigned char> d_mask;
    // the temporaries go away on return: no failure leaves work on them queued
    auto fail = [&]() { avt_set_error(std::string(who) + ": device call failed"); (void)hipStreamSynchronize(rf->stream); return 1; };
    if (d_depth.reserve(batch * npix) || d_mask.reserve(batch * npix) || score_begin(rf)) return fail();
    for (int i0 = 0; i0 < n; i0 += batch) {
        const int k = std::min(batch, n - i0);
        if (hipMemcpyAsync(d_depth, depth + i0 * npix, k * npix * sizeof(float), hipMemcpyHostToDevice, rf->stream) != hipSuccess ||
            hipMemcpyAsync(d_mask, mask + i0 * npix, k * npix, hipMemcpyHostToDevice, rf->stream) != hipSuccess ||
            avt_rforest_launch_score(rf, d_depth, d_mask, k, rows, cols, stride, rf->d_score, rf->d_score_bad) ||
            hipStreamSynchronize(rf->stream) != hipSuccess)   // the next batch goes into the same buffers
            return fail();
    }
    return score_commit(rf, who, n, rows, cols, stride);
}

int score_rendered_impl(avt_rforest* rf, avt_renderer* r, int stride) {
    const char* who = "avt_rforest_score_rendered";
    if (!rf) { avt_set_error(std::string(who) + ": null forest"); return 1; }
    if (stride < 1) { avt_set_error(std::string(who) + ": needs stride >= 1"); return 1; }
    if (rf->device < 0) { avt_set_error(kHostOnly); return 1; }
    if (!r) { avt_set_error(std::string(who) + ": null renderer"); return 1; }
    const float* depth = nullptr;
    const unsigned char* mask = nullptr;
    int n = 0, w = 0, h = 0;
    if (avt_renderer_images_for(r, rf->stream, &depth, &mask, &n, &w, &h)) return 1;
    // from here the forest's stream waits for the renderer; every path below drains it before it returns, as that function asks
    hipPointerAttribute_t at;
    int rc = 0;
    if (hipPointerGetAttributes(&at, depth) != hipSuccess || at.device != rf->device) {
        (void)hipGetLastError();
        avt_set_error(std::string(who) + ": the forest and the renderer are on different devices");
        rc = 1;
    }
    if (hipSetDevice(rf->device) != hipSuccess) rc = 1;
    if (!rc && (h >= 32768 || w >= 32768)) { avt_set_error(std::string(who) + ": images of at most 32767 rows and columns"); rc = 1; }
    if (!rc && (score_begin(rf) || avt_rforest_launch_score(rf, depth, mask, n, h, w, stride, rf->d_score, rf->d_score_bad))) {
        avt_set_error(std::string(who) + ": device call failed");
        rc = 1;
    }
    if (rc) { (void)hipStreamSynchronize(rf->stream); return 1; }
    return score_commit(rf, who, n, h, w, stride);      // the images were read where they lie; the stream has finished
}

int score_get_impl(avt_rforest* rf, long long* confusion, long long* n_images, long long* n_pixels) {
    if (!rf) { avt_set_error("avt_rforest_score_get: null forest"); return 1; }
    const size_t cells = (size_t)(rf->num_parts + 1) * (rf->num_parts + 1);
    if (confusion) {
        if (rf->score_conf.empty()) std::fill(confusion, confusion + cells, 0ll);
        else std::copy(rf->score_conf.begin(), rf->score_conf.end(), confusion);
    }
    if (n_images) *n_images = rf->score_images;
    if (n_pixels) *n_pixels = rf->score_pixels;
    return 0;
}

}  // namespace

// ---- exported entry points: no C++ exception crosses the C ABI
extern "C" {

int avt_rforest_create(const avt_rtree* const* trees, int n_trees, int device, avt_rforest** out) {
    return avt_guard("avt_rforest_create", [&]() -> int { return create_impl(trees, n_trees, device, out); });
}

void avt_rforest_destroy(avt_rforest* rf) {
    if (!rf) return;
    avt_label_teardown(rf);
    delete rf;
}

int avt_rforest_info(const avt_rforest* rf, int* n_trees, int* num_parts, int* part_map_len, int* part_map_type, int* total_nodes, int* total_leafs) {
    if (!rf) { avt_set_error("avt_rforest_info: null forest"); return 1; }
    if (n_trees) *n_trees = rf->n_trees;
    if (num_parts) *num_parts = rf->num_parts;
    if (part_map_len) *part_map_len = (int)rf->part_map.size();
    if (part_map_type) *part_map_type = rf->part_map_type;
    if (total_nodes) *total_nodes = (int)rf->nodes.size();
    if (total_leafs) *total_leafs = (int)(rf->leaf.size() / rf->num_parts);
    return 0;
}

int avt_rforest_predict(avt_rforest* rf, const float* depth, int rows, int cols, float* dist_out) {
    return avt_guard("avt_rforest_predict", [&]() -> int { return avt_label_predict_dist(rf, kForest, true, depth, rows, cols, dist_out, launch_dist); });
}

int avt_rforest_predict_best(avt_rforest* rf, const float* depth, int rows, int cols, int interval, int tlx, int tly, int brx, int bry, int fill,
                             unsigned char* labels_out) {
    return avt_guard("avt_rforest_predict_best", [&]() -> int { return predict_best_impl(rf, depth, rows, cols, interval, tlx, tly, brx, bry, fill, labels_out); });
}

int avt_rforest_images_upload(avt_rforest* rf, int n_images, int rows, int cols, const float* depth) {
    return avt_guard("avt_rforest_images_upload", [&]() -> int { return avt_label_images_upload(rf, kForest, kMaxImages, n_images, rows, cols, depth); });
}

int avt_rforest_predict_best_resident_boxes(avt_rforest* rf, int interval, const int* boxes, int fill) {
    return avt_guard("avt_rforest_predict_best_resident_boxes", [&]() -> int { return avt_label_predict_resident_boxes(rf, kForest, interval, boxes, fill, launch_boxes); });
}

int avt_rforest_predict_best_from_bgsub(avt_rforest* rf, avt_bgsub* bg, int interval, int fill) {
    return avt_guard("avt_rforest_predict_best_from_bgsub", [&]() -> int { return avt_label_predict_from_bgsub(rf, kForest, kMaxImages, bg, interval, fill, launch_boxes); });
}

int avt_rforest_labels_download(avt_rforest* rf, int image, unsigned char* labels_out) {
    return avt_guard("avt_rforest_labels_download", [&]() -> int { return avt_label_labels_download(rf, kForest, image, labels_out); });
}

int avt_rforest_labels_download_all(avt_rforest* rf, unsigned char* labels_out) {
    return avt_guard("avt_rforest_labels_download_all", [&]() -> int { return avt_label_labels_download_all(rf, kForest, labels_out); });
}

int avt_rforest_sync(avt_rforest* rf) { return avt_label_sync(rf, kForest, true); }      // refuses a host-only forest

int avt_rforest_labels_upload(avt_rforest* rf, int n_images, int rows, int cols, const unsigned char* labels) {
    return avt_guard("avt_rforest_labels_upload", [&]() -> int { return avt_post_labels_upload(rf, "avt_rforest_labels_upload", n_images, rows, cols, labels); });
}

int avt_rforest_post_process_resident(avt_rforest* rf, int interval, const int* boxes, double dist_to_pre_weight) {
    return avt_guard("avt_rforest_post_process_resident", [&]() -> int { return avt_post_resident(rf, "avt_rforest_post_process_resident", interval, boxes, dist_to_pre_weight); });
}

int avt_rforest_post_process_from_bgsub(avt_rforest* rf, avt_bgsub* bg, int interval, double dist_to_pre_weight) {
    return avt_guard("avt_rforest_post_process_from_bgsub", [&]() -> int { return avt_post_from_bgsub(rf, bg, "avt_rforest_post_process_from_bgsub", interval, dist_to_pre_weight); });
}

int avt_rforest_com_pre_set(avt_rforest* rf, int first, int n, const double* com, const unsigned char* valid) {
    return avt_guard("avt_rforest_com_pre_set", [&]() -> int { return avt_label_com_pre_set(rf, kForest, first, n, com, valid); });
}

int avt_rforest_com_pre_get(avt_rforest* rf, int first, int n, double* com, unsigned char* valid) {
    return avt_guard("avt_rforest_com_pre_get", [&]() -> int { return avt_label_com_pre_get(rf, kForest, first, n, com, valid); });
}

int avt_rforest_score_reset(avt_rforest* rf) {
    if (!rf) { avt_set_error("avt_rforest_score_reset: null forest"); return 1; }
    rf->score_conf.clear();
    rf->score_images = rf->score_pixels = 0;
    return 0;
}

int avt_rforest_score_images(avt_rforest* rf, int n_images, int rows, int cols, const float* depth, const unsigned char* part_mask, int stride) {
    return avt_guard("avt_rforest_score_images", [&]() -> int { return score_images_impl(rf, n_images, rows, cols, depth, part_mask, stride); });
}

int avt_rforest_score_rendered(avt_rforest* rf, struct avt_renderer* r, int stride) {
    return avt_guard("avt_rforest_score_rendered", [&]() -> int { return score_rendered_impl(rf, r, stride); });
}

int avt_rforest_score_get(avt_rforest* rf, long long* confusion, long long* n_images, long long* n_pixels) {
    return avt_guard("avt_rforest_score_get", [&]() -> int { return score_get_impl(rf, confusion, n_images, n_pixels); });
}

}  // extern "C"
