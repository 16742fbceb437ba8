// avt_rtree_train.cpp — host driver of the forest trainer (include/avt_rtree_train.h): image ingestion, the level loop with
// the leaf rules of trainFromNode (RTree.cpp:2501-2647), the renumbering into the reference's depth-first order, and
// trainTransfer's normalisation (:3408-3419).  The kernels are in avt_rtree_train.hip.
#include "avt_rtree_train.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "avt_internal.h"

namespace {

// the sample arrays grow by doubling and keep their contents (DevBuf::grow)
struct Samples {
    DevBuf<int> img, xy;
    DevBuf<float> d;
    DevBuf<unsigned char> lab;
    int grow(size_t n, size_t keep, hipStream_t s) { return img.grow(n, keep, s) || xy.grow(n, keep, s) || d.grow(n, keep, s) || lab.grow(n, keep, s); }
    RtSamples dev() const { return RtSamples{img.p, xy.p, d.p, lab.p}; }
};

// what the level loop learned about one node
struct HostNode {
    bool leaf = true;
    float feat[5] = {0, 0, 0, 0, 0};
    int child = -1;                  // split: index of the left child in the next level (right child: child + 1)
    std::vector<float> dist;         // leaf: (float)count_p / (float)n
};

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

struct avt_rtree_trainer {
    int device = 0;
    avt_rtree_train_params p{};
    hipStream_t stream = nullptr;
    std::vector<RtImg> imgs;          // host copy of the crop table
    DevBuf<RtImg> d_imgs;
    DevBuf<float> store;              // crops
    long long store_used = 0;
    Samples s;                        // as chosen; the level loop works on copies
    long long n_samples = 0;
};

namespace {

int check_args(const avt_rtree_trainer* tr, int n, int rows, int cols, const void* depth, const void* mask, const char* who) {
    if (!tr || n <= 0 || rows <= 0 || cols <= 0 || rows >= 32768 || cols >= 32768 || !depth || !mask) {
        avt_set_error(std::string(who) + ": bad arguments (n >= 1, 1 <= rows, cols < 32768, non-null images)");
        return 1;
    }
    return 0;
}

// n images from the host (kind hipMemcpyHostToDevice) or from device buffers (hipMemcpyDeviceToDevice, already ordered after
// their producer on tr->stream).  Nothing of the trainer changes unless every image passes the checks.
int add_batch(avt_rtree_trainer* tr, int n, int rows, int cols, const float* depth, const unsigned char* mask, hipMemcpyKind kind) {
    hipStream_t st = tr->stream;
    const size_t npix = (size_t)rows * cols;
    DevBuf<float> d_depth;
    DevBuf<unsigned char> d_mask;
    DevBuf<int> d_scan, d_scratch;
    DevBuf<long long> d_off;
    // the temporaries above and the host arrays below go away on return: no failure leaves work on them queued
    auto fail = [&](const std::string& what) { avt_set_error("avt_rtree_trainer_add_images: " + what); (void)hipStreamSynchronize(st); return 1; };
    if (d_depth.reserve(n * npix) || d_mask.reserve(n * npix) || d_scan.reserve((size_t)n * 7) || d_scratch.reserve(n * npix) || d_off.reserve(n))
        return fail("out of device memory");
    if (hipMemcpyAsync(d_depth, depth, n * npix * sizeof(float), kind, st) != hipSuccess ||
        hipMemcpyAsync(d_mask, mask, n * npix, kind, st) != hipSuccess) return fail("image copy failed");
    if (rt_launch_img_scan(st, d_depth, d_mask, n, rows, cols, d_scan)) return fail("kernel launch failed");
    std::vector<int> scan((size_t)n * 7);
    if (hipMemcpyAsync(scan.data(), d_scan, scan.size() * sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) return fail("scan failed");
    bool bad_label = false, bad_depth = false;
    for (int i = 0; i < n; ++i) { bad_label |= scan[7 * (size_t)i + 5] >= tr->p.num_parts; bad_depth |= scan[7 * (size_t)i + 6] != 0; }
    if (bad_label) return fail("a part-mask label is >= num_parts (and not 255)");
    if (bad_depth) return fail("depth must be finite and >= 0");
    // crops and sample offsets of this batch
    const int base = (int)tr->imgs.size();
    std::vector<RtImg> bi(n);
    std::vector<long long> off(n);
    long long add_pix = 0, add_s = 0;
    for (int i = 0; i < n; ++i) {
        const int* q = &scan[7 * (size_t)i];
        RtImg m{};
        m.off = tr->store_used + add_pix;
        if (q[2] >= 0) { m.x0 = q[0]; m.y0 = q[1]; m.w = q[2] - q[0] + 1; m.h = q[3] - q[1] + 1; }
        add_pix += (long long)m.w * m.h;
        bi[i] = m;
        off[i] = tr->n_samples + add_s;
        add_s += std::min(q[4], tr->p.num_points_per_image);
    }
    if (tr->store.grow((size_t)(tr->store_used + add_pix) + 1, (size_t)tr->store_used, st) ||
        tr->d_imgs.grow(tr->imgs.size() + n, tr->imgs.size(), st) || tr->s.grow((size_t)(tr->n_samples + add_s) + 1, (size_t)tr->n_samples, st))
        return 1;
    if (hipMemcpyAsync(tr->d_imgs.p + base, bi.data(), n * sizeof(RtImg), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(d_off, off.data(), n * sizeof(long long), hipMemcpyHostToDevice, st) != hipSuccess) return fail("upload failed");
    if (rt_launch_crop(st, d_depth, n, rows, cols, tr->d_imgs.p + base, tr->store.p) ||
        rt_launch_select(st, d_depth, d_mask, n, rows, cols, tr->p.num_points_per_image, tr->p.seed, base, d_off, d_scratch, tr->s.dev()))
        return fail("kernel launch failed");
    if (hipStreamSynchronize(st) != hipSuccess) return fail("stream failed");   // bi / off live on this frame
    tr->imgs.insert(tr->imgs.end(), bi.begin(), bi.end());
    tr->store_used += add_pix;
    tr->n_samples += add_s;
    return 0;
}

int train(avt_rtree_trainer* tr, int part_map_len, const int* part_map, int part_map_type, avt_rtree** out, avt_rtree_train_stats* stats) {
    const auto t_run = std::chrono::steady_clock::now();
    const avt_rtree_train_params& p = tr->p;
    const int P = p.num_parts, T = p.min_samples_per_feature, F = p.num_features;
    const long long N = tr->n_samples;
    hipStream_t st = tr->stream;
    RtTrainArgs args{p.seed, P, T, F, p.max_probe_offset};
    avt_rtree_train_stats sx{};
    sx.n_images = (int)tr->imgs.size();
    sx.n_samples = N;

    Samples a, b;
    DevBuf<RtNode> d_nodes;
    DevBuf<int> d_counts, d_list;
    DevBuf<RtChunk> d_chunks;
    DevBuf<RtRes> d_res;
    if (a.grow((size_t)N, 0, st) || b.grow((size_t)N, 0, st)) return 1;
    AVT_HIP(hipMemcpyAsync(a.img.p, tr->s.img.p, N * sizeof(int), hipMemcpyDeviceToDevice, st));
    AVT_HIP(hipMemcpyAsync(a.xy.p, tr->s.xy.p, N * sizeof(int), hipMemcpyDeviceToDevice, st));
    AVT_HIP(hipMemcpyAsync(a.d.p, tr->s.d.p, N * sizeof(float), hipMemcpyDeviceToDevice, st));
    AVT_HIP(hipMemcpyAsync(a.lab.p, tr->s.lab.p, N, hipMemcpyDeviceToDevice, st));

    std::vector<std::vector<HostNode>> levels;
    std::vector<RtNode> level{RtNode{0, (int)N, 1ull}};
    std::vector<char> forced{0};
    for (int L = 0; !level.empty(); ++L) {
        if (L >= AVT_RTREE_TRAIN_MAX_DEPTH) { avt_set_error("avt_rtree_trainer_run: level limit exceeded"); return 1; }
        const auto t_level = std::chrono::steady_clock::now();
        const int M = (int)level.size(), depth = p.max_tree_depth - L;
        // which nodes are searched: not a forced leaf, depth > 1, n > min_samples (RTree.cpp:2506)
        std::vector<int> large, small;
        long long evals = 0;
        for (int m = 0; m < M; ++m) {
            const int n = level[m].end - level[m].start;
            if (forced[m] || depth <= 1 || n <= p.min_samples) continue;
            (n >= 2048 ? large : small).push_back(m);
            evals += (long long)n * F;
        }
        const int nl = (int)large.size(), ns = (int)small.size();
        auto chunking = [&](int cnt, int target, int& nch, int& fch) {
            nch = cnt ? std::max(1, std::min(F, (target + cnt - 1) / cnt)) : 1;
            fch = (F + nch - 1) / nch;
            nch = (F + fch - 1) / fch;
        };
        int nch_l, fch_l, nch_s, fch_s;
        chunking(nl, 2048, nch_l, fch_l);
        chunking(ns, 8192, nch_s, fch_s);
        std::vector<int> list(large);
        list.insert(list.end(), small.begin(), small.end());
        if (d_nodes.grow(M, 0, st) || d_counts.grow((size_t)M * P, 0, st) || d_res.grow(M, 0, st) || d_list.grow(list.size() + 1, 0, st) ||
            d_chunks.grow((size_t)nl * nch_l + (size_t)ns * nch_s + 1, 0, st))
            return 1;
        AVT_HIP(hipMemcpyAsync(d_nodes.p, level.data(), M * sizeof(RtNode), hipMemcpyHostToDevice, st));
        if (!list.empty()) AVT_HIP(hipMemcpyAsync(d_list.p, list.data(), list.size() * sizeof(int), hipMemcpyHostToDevice, st));
        int lrc = rt_launch_count(st, d_nodes.p, M, a.lab.p, P, d_counts.p);
        RtChunk* ch_s = d_chunks.p + (size_t)nl * nch_l;
        if (nl) lrc = lrc || rt_launch_search(st, true, d_list.p, nl, nch_l, fch_l, d_nodes.p, d_counts.p, a.dev(), tr->d_imgs.p, tr->store.p, args, d_chunks.p) ||
                      rt_launch_choose(st, d_list.p, nl, nch_l, d_nodes.p, d_chunks.p, args, d_res.p);
        if (ns) lrc = lrc || rt_launch_search(st, false, d_list.p + nl, ns, nch_s, fch_s, d_nodes.p, d_counts.p, a.dev(), tr->d_imgs.p, tr->store.p, args, ch_s) ||
                      rt_launch_choose(st, d_list.p + nl, ns, nch_s, d_nodes.p, ch_s, args, d_res.p);
        if (!list.empty()) lrc = lrc || rt_launch_partition(st, d_list.p, (int)list.size(), d_nodes.p, d_res.p, a.dev(), b.dev(), tr->d_imgs.p, tr->store.p);
        if (lrc) { avt_set_error("avt_rtree_trainer_run: kernel launch failed"); return 1; }
        std::vector<RtRes> res(M);
        std::vector<int> counts((size_t)M * P);
        AVT_HIP(hipMemcpyAsync(res.data(), d_res.p, M * sizeof(RtRes), hipMemcpyDeviceToHost, st));
        AVT_HIP(hipMemcpyAsync(counts.data(), d_counts.p, counts.size() * sizeof(int), hipMemcpyDeviceToHost, st));
        AVT_HIP(hipStreamSynchronize(st));                 // the one wait of the level
        std::vector<char> searched(M, 0);
        for (int m : list) searched[m] = 1;
        std::vector<HostNode> hn(M);
        std::vector<RtNode> next;
        std::vector<char> next_forced;
        for (int m = 0; m < M; ++m) {
            const RtNode& nd = level[m];
            const int n = nd.end - nd.start;
            HostNode& h = hn[m];
            const RtRes& r = res[m];
            if (searched[m] && r.f >= 0 && r.nleft > 0 && r.nleft < n) {
                h.leaf = false;
                std::memcpy(h.feat, r.feat, sizeof h.feat);
                h.child = (int)next.size();
                next.push_back(RtNode{nd.start, nd.start + r.nleft, 2 * nd.key});
                next.push_back(RtNode{nd.start + r.nleft, nd.end, 2 * nd.key + 1});
                const char zero = r.gain == 0.0;          // both children become leaves at once (:2640-2642)
                next_forced.push_back(zero);
                next_forced.push_back(zero);
            } else {
                h.dist.resize(P);
                for (int q = 0; q < P; ++q) h.dist[q] = (float)counts[(size_t)m * P + q] / (float)n;
            }
        }
        levels.push_back(std::move(hn));
        sx.level_nodes[L] = M;
        sx.level_searched[L] = (int)list.size();
        sx.level_large[L] = nl;
        sx.level_evals[L] = evals;
        sx.level_ms[L] = ms_since(t_level);
        sx.n_levels = L + 1;
        std::swap(a, b);
        level.swap(next);
        forced.swap(next_forced);
    }

    // the reference's numbering: a split node appends its two children, then the left subtree, then the right (:2632-2646)
    size_t total = 0;
    for (auto& l : levels) total += l.size();
    std::vector<float> feature(5 * total, 0.f), leaf_data;
    std::vector<int> links(3 * total, -1);
    int next_id = 1, next_leaf = 0;
    struct Walk {
        std::vector<std::vector<HostNode>>& lv;
        std::vector<float>& feature;
        std::vector<int>& links;
        std::vector<float>& leaf_data;
        int& next_id;
        int& next_leaf;
        void visit(int L, int i, int id) {
            const HostNode& h = lv[L][i];
            if (h.leaf) {
                links[3 * (size_t)id + 2] = next_leaf++;
                leaf_data.insert(leaf_data.end(), h.dist.begin(), h.dist.end());
                return;
            }
            const int l = next_id++, r = next_id++;
            links[3 * (size_t)id] = l;
            links[3 * (size_t)id + 1] = r;
            std::copy(h.feat, h.feat + 5, &feature[5 * (size_t)id]);
            visit(L + 1, h.child, l);
            visit(L + 1, h.child + 1, r);
        }
    } walk{levels, feature, links, leaf_data, next_id, next_leaf};
    walk.visit(0, 0, 0);
    avt_rtree_desc desc{next_id, next_leaf, P, feature.data(), links.data(), leaf_data.data(), part_map_len, part_map, part_map_type};
    if (avt_rtree_create(&desc, tr->device, out)) return 1;
    sx.n_nodes = next_id;
    sx.n_leafs = next_leaf;
    sx.total_ms = ms_since(t_run);
    if (stats) *stats = sx;
    return 0;
}

// trainTransfer's counts of n images (host or device buffers, `kind`) added to rt->d_tcount; a label >= num_parts drops the
// batch's counts and fails
int transfer_add(avt_rtree* rt, int n, int rows, int cols, const float* depth, const unsigned char* mask, hipMemcpyKind kind, const char* who) {
    const int P = rt->num_parts, nl = (int)rt->leaf_best.size();
    const size_t ncnt = std::max<size_t>(1, (size_t)nl * P);
    AVT_HIP(hipSetDevice(rt->device));
    if (!rt->d_tcount) {
        if (rt->d_tcount.reserve(ncnt)) return 1;
        AVT_HIP(hipMemsetAsync(rt->d_tcount, 0, ncnt * sizeof(unsigned long long), rt->stream));
    }
    const size_t npix = (size_t)rows * cols;
    const int batch = (int)std::max<size_t>(1, std::min<size_t>(n, ((size_t)256 << 20) / (npix * 5)));
    DevBuf<float> d_depth;
    DevBuf<unsigned char> d_mask;
    DevBuf<unsigned long long> d_cnt;
    DevBuf<int> d_bad;
    // the temporaries go away on return: no failure leaves work on them queued
    auto fail = [&]() { avt_set_error(std::string(who) + ": device call failed"); (void)hipStreamSynchronize(rt->stream); return 1; };
    if (d_depth.reserve(batch * npix) || d_mask.reserve(batch * npix) || d_cnt.reserve(ncnt) || d_bad.reserve(1) ||
        hipMemsetAsync(d_cnt, 0, ncnt * sizeof(unsigned long long), rt->stream) != hipSuccess ||
        hipMemsetAsync(d_bad, 0, sizeof(int), rt->stream) != hipSuccess) return fail();
    for (int i0 = 0; i0 < n; i0 += batch) {
        const int k = std::min(batch, n - i0);
        if (hipMemcpyAsync(d_depth, depth + i0 * npix, k * npix * sizeof(float), kind, rt->stream) != hipSuccess ||
            hipMemcpyAsync(d_mask, mask + i0 * npix, k * npix, kind, rt->stream) != hipSuccess ||
            rt_launch_transfer(rt->stream, rt->d_nodes, d_depth, d_mask, k, rows, cols, P, d_cnt, d_bad) ||
            hipStreamSynchronize(rt->stream) != hipSuccess)   // the next batch goes into the same buffers
            return fail();
    }
    int bad = 0;
    if (hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, rt->stream) != hipSuccess || hipStreamSynchronize(rt->stream) != hipSuccess) return fail();
    if (bad) { avt_set_error(std::string(who) + ": a part-mask label is >= num_parts (and not 255); the batch's counts were dropped"); return 1; }
    // the batch is good: add its integer counts to those kept since the last finish
    std::vector<unsigned long long> add(ncnt), acc(ncnt);
    if (hipMemcpyAsync(add.data(), d_cnt, ncnt * sizeof(unsigned long long), hipMemcpyDeviceToHost, rt->stream) != hipSuccess ||
        hipMemcpyAsync(acc.data(), rt->d_tcount, ncnt * sizeof(unsigned long long), hipMemcpyDeviceToHost, rt->stream) != hipSuccess ||
        hipStreamSynchronize(rt->stream) != hipSuccess) return fail();
    for (size_t i = 0; i < ncnt; ++i) acc[i] += add[i];
    if (hipMemcpyAsync(rt->d_tcount, acc.data(), ncnt * sizeof(unsigned long long), hipMemcpyHostToDevice, rt->stream) != hipSuccess ||
        hipStreamSynchronize(rt->stream) != hipSuccess) return fail();
    return 0;
}

// count / sum for every leaf with a count (RTree.cpp:3408-3419), the counts start over
int transfer_finish(avt_rtree* rt, int* n_unvisited) {
    const int P = rt->num_parts, nl = (int)rt->leaf_best.size();
    int unvisited = nl;
    if (rt->d_tcount) {
        AVT_HIP(hipSetDevice(rt->device));
        const size_t ncnt = std::max<size_t>(1, (size_t)nl * P);
        std::vector<unsigned long long> cnt(ncnt);
        AVT_HIP(hipMemcpyAsync(cnt.data(), rt->d_tcount, ncnt * sizeof(unsigned long long), hipMemcpyDeviceToHost, rt->stream));
        AVT_HIP(hipStreamSynchronize(rt->stream));
        rt->d_tcount.release();
        unvisited = 0;
        for (int l = 0; l < nl; ++l) {
            unsigned long long sum = 0;
            for (int q = 0; q < P; ++q) sum += cnt[(size_t)l * P + q];
            if (sum > 0) {
                for (int q = 0; q < P; ++q) rt->leaf_data[(size_t)l * P + q] = (float)cnt[(size_t)l * P + q] / (float)sum;
            } else {
                ++unvisited;
            }
        }
    }
    if (n_unvisited) *n_unvisited = unvisited;
    return avt_rtree_refresh_leaves(rt);
}

int root_histograms(avt_rtree_trainer* tr, int nf, int* hist, float* minmax) {
    const int P = tr->p.num_parts, T = tr->p.min_samples_per_feature;
    hipStream_t st = tr->stream;
    RtTrainArgs args{tr->p.seed, P, T, nf, tr->p.max_probe_offset};
    const RtNode root{0, (int)tr->n_samples, 1ull};
    const int zero = 0;
    DevBuf<RtNode> d_node;
    DevBuf<int> d_counts, d_list, d_hist;
    DevBuf<float> d_mm;
    DevBuf<RtChunk> d_ch;
    const size_t nh = (size_t)nf * P * T;
    int rc = 0;
    if (d_node.reserve(1) || d_counts.reserve(P) || d_list.reserve(1) || d_hist.reserve(nh) || d_mm.reserve(2 * (size_t)nf) || d_ch.reserve(nf) ||
        hipMemcpyAsync(d_node, &root, sizeof(RtNode), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(d_list, &zero, sizeof(int), hipMemcpyHostToDevice, st) != hipSuccess ||
        rt_launch_count(st, d_node, 1, tr->s.lab.p, P, d_counts) ||
        rt_launch_search(st, tr->n_samples >= 2048, d_list, 1, nf, 1, d_node, d_counts, tr->s.dev(), tr->d_imgs.p, tr->store.p, args, d_ch, d_hist, d_mm) ||
        hipMemcpyAsync(hist, d_hist, nh * sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
        (minmax && hipMemcpyAsync(minmax, d_mm, 2 * (size_t)nf * sizeof(float), hipMemcpyDeviceToHost, st) != hipSuccess))
        rc = 1;
    if (hipStreamSynchronize(st) != hipSuccess) rc = 1;   // on every path: the temporaries, `root` and `zero` go away on return
    if (rc) avt_set_error("avt_rtree_trainer_root_histograms: device call failed");
    return rc;
}

}  // namespace

extern "C" {

int avt_rtree_trainer_create(int device, const avt_rtree_train_params* p, avt_rtree_trainer** out) {
    return avt_guard("avt_rtree_trainer_create", [&]() -> int {
        if (!p || !out || p->num_parts < 1 || p->num_parts > 127 || p->num_points_per_image < 1 || p->num_features < 1 ||
            !(p->max_probe_offset > 0.5f) || std::isinf(p->max_probe_offset) || p->min_samples < 0 || p->max_tree_depth < 1 ||
            p->max_tree_depth > AVT_RTREE_TRAIN_MAX_DEPTH || p->min_samples_per_feature < 1 || (long long)p->num_parts * p->min_samples_per_feature > 8192) {
            avt_set_error("avt_rtree_trainer_create: bad parameters (1 <= num_parts <= 127, points / features / T >= 1, max_probe_offset > 0.5, "
                          "min_samples >= 0, 1 <= max_tree_depth <= 64, num_parts x T <= 8192)");
            return 1;
        }
        AVT_HIP(hipSetDevice(device));
        // k_rt_search's dynamic LDS: decided here, so that no accepted parameter set fails in run().  The attribute is raised to
        // the largest request the check above admits (P = 1, T = 8192 in the 256-thread form), or to the device's limit if lower.
        int lds_limit = 0;
        AVT_HIP(hipDeviceGetAttribute(&lds_limit, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
        size_t lds_most = 0;
        for (int q = 1; q <= 127; ++q) lds_most = std::max(lds_most, rt_search_lds_bytes(q, 8192 / q, true));
        const size_t lds_need = rt_search_lds_bytes(p->num_parts, p->min_samples_per_feature, true);
        if (lds_need > (size_t)lds_limit || rt_search_set_attributes(std::min(lds_most, (size_t)lds_limit))) {
            (void)hipGetLastError();
            avt_set_error("avt_rtree_trainer_create: num_parts x T = " + std::to_string(p->num_parts) + " x " + std::to_string(p->min_samples_per_feature) +
                          " needs " + std::to_string(lds_need) + " bytes of LDS per workgroup, the device grants " + std::to_string(lds_limit));
            return 1;
        }
        avt_rtree_trainer* tr = new avt_rtree_trainer();
        tr->device = device;
        tr->p = *p;
        if (hipStreamCreateWithFlags(&tr->stream, hipStreamNonBlocking) != hipSuccess) {
            delete tr;
            avt_set_error("avt_rtree_trainer_create: stream creation failed");
            return 1;
        }
        *out = tr;
        return 0;
    });
}

void avt_rtree_trainer_destroy(avt_rtree_trainer* tr) {
    if (!tr) return;
    (void)hipSetDevice(tr->device);
    if (tr->stream) (void)hipStreamSynchronize(tr->stream);
    // the buffers go with `delete`, after the stream: it has just been drained, so nothing is queued on them either way
    if (tr->stream) (void)hipStreamDestroy(tr->stream);
    delete tr;
}

int avt_rtree_trainer_add_images(avt_rtree_trainer* tr, int n, int rows, int cols, const float* depth, const unsigned char* mask) {
    return avt_guard("avt_rtree_trainer_add_images", [&]() -> int {
        if (check_args(tr, n, rows, cols, depth, mask, "avt_rtree_trainer_add_images")) return 1;
        AVT_HIP(hipSetDevice(tr->device));
        // batches of at most ~512 MB of temporaries; image indices and samples do not depend on the batching
        const size_t npix = (size_t)rows * cols;
        const int batch = (int)std::max<size_t>(1, std::min<size_t>(n, ((size_t)512 << 20) / (npix * 9)));
        for (int i0 = 0; i0 < n; i0 += batch) {
            const int k = std::min(batch, n - i0);
            if (add_batch(tr, k, rows, cols, depth + i0 * npix, mask + i0 * npix, hipMemcpyHostToDevice)) return 1;
        }
        return 0;
    });
}

int avt_rtree_trainer_info(const avt_rtree_trainer* tr, int* n_images, long long* n_samples) {
    if (!tr) { avt_set_error("avt_rtree_trainer_info: null trainer"); return 1; }
    if (n_images) *n_images = (int)tr->imgs.size();
    if (n_samples) *n_samples = tr->n_samples;
    return 0;
}

int avt_rtree_trainer_samples(avt_rtree_trainer* tr, int* image, int* x, int* y, unsigned char* label) {
    return avt_guard("avt_rtree_trainer_samples", [&]() -> int {
        if (!tr) { avt_set_error("avt_rtree_trainer_samples: null trainer"); return 1; }
        const size_t n = (size_t)tr->n_samples;
        if (!n) return 0;
        AVT_HIP(hipSetDevice(tr->device));
        std::vector<int> xy(n);
        if (image) AVT_HIP(hipMemcpyAsync(image, tr->s.img.p, n * sizeof(int), hipMemcpyDeviceToHost, tr->stream));
        AVT_HIP(hipMemcpyAsync(xy.data(), tr->s.xy.p, n * sizeof(int), hipMemcpyDeviceToHost, tr->stream));
        if (label) AVT_HIP(hipMemcpyAsync(label, tr->s.lab.p, n, hipMemcpyDeviceToHost, tr->stream));
        AVT_HIP(hipStreamSynchronize(tr->stream));
        for (size_t i = 0; i < n; ++i) {
            if (x) x[i] = xy[i] & 0xffff;
            if (y) y[i] = xy[i] >> 16;
        }
        return 0;
    });
}

int avt_rtree_trainer_run(avt_rtree_trainer* tr, int part_map_len, const int* part_map, int part_map_type, avt_rtree** out, avt_rtree_train_stats* stats) {
    return avt_guard("avt_rtree_trainer_run", [&]() -> int {
        if (!tr || !out || part_map_len < 0 || (part_map_len > 0 && !part_map)) { avt_set_error("avt_rtree_trainer_run: bad arguments"); return 1; }
        if (tr->n_samples <= 0) { avt_set_error("avt_rtree_trainer_run: no samples (add images with labelled pixels first)"); return 1; }
        if (tr->n_samples >= (1ll << 31)) { avt_set_error("avt_rtree_trainer_run: more than 2^31 - 1 samples"); return 1; }
        AVT_HIP(hipSetDevice(tr->device));
        return train(tr, part_map_len, part_map, part_map_type, out, stats);
    });
}

int avt_rtree_transfer_images(avt_rtree* rt, int n, int rows, int cols, const float* depth, const unsigned char* mask, int* n_unvisited) {
    return avt_guard("avt_rtree_transfer_images", [&]() -> int {
        if (!rt || rt->device < 0 || !rt->d_nodes) { avt_set_error("avt_rtree_transfer_images: needs a tree on a device"); return 1; }
        avt_rtree_trainer probe;
        if (check_args(&probe, n, rows, cols, depth, mask, "avt_rtree_transfer_images")) return 1;
        if (transfer_add(rt, n, rows, cols, depth, mask, hipMemcpyHostToDevice, "avt_rtree_transfer_images")) return 1;
        return transfer_finish(rt, n_unvisited);
    });
}

int avt_rtree_transfer_rendered(avt_rtree* rt, avt_renderer* r) {
    return avt_guard("avt_rtree_transfer_rendered", [&]() -> int {
        if (!rt || rt->device < 0 || !rt->d_nodes || !r) { avt_set_error("avt_rtree_transfer_rendered: needs a tree on a device and a renderer"); return 1; }
        AVT_HIP(hipSetDevice(rt->device));
        const float* depth = nullptr;
        const unsigned char* mask = nullptr;
        int n = 0, w = 0, h = 0;
        if (avt_renderer_images_for(r, rt->stream, &depth, &mask, &n, &w, &h)) return 1;
        return transfer_add(rt, n, h, w, depth, mask, hipMemcpyDeviceToDevice, "avt_rtree_transfer_rendered");
    });
}

int avt_rtree_transfer_finish(avt_rtree* rt, int* n_unvisited) {
    return avt_guard("avt_rtree_transfer_finish", [&]() -> int {
        if (!rt || rt->device < 0 || !rt->d_nodes) { avt_set_error("avt_rtree_transfer_finish: needs a tree on a device"); return 1; }
        return transfer_finish(rt, n_unvisited);
    });
}

int avt_rtree_trainer_add_rendered(avt_rtree_trainer* tr, avt_renderer* r) {
    return avt_guard("avt_rtree_trainer_add_rendered", [&]() -> int {
        if (!tr || !r) { avt_set_error("avt_rtree_trainer_add_rendered: null argument"); return 1; }
        AVT_HIP(hipSetDevice(tr->device));
        const float* depth = nullptr;
        const unsigned char* mask = nullptr;
        int n = 0, w = 0, h = 0;
        if (avt_renderer_images_for(r, tr->stream, &depth, &mask, &n, &w, &h)) return 1;
        if (check_args(tr, n, h, w, depth, mask, "avt_rtree_trainer_add_rendered")) return 1;
        return add_batch(tr, n, h, w, depth, mask, hipMemcpyDeviceToDevice);
    });
}

int avt_rtree_trainer_root_histograms(avt_rtree_trainer* tr, int n_features, int* hist, float* minmax) {
    return avt_guard("avt_rtree_trainer_root_histograms", [&]() -> int {
        if (!tr || n_features < 1 || !hist) { avt_set_error("avt_rtree_trainer_root_histograms: bad arguments"); return 1; }
        if (tr->n_samples <= 0) { avt_set_error("avt_rtree_trainer_root_histograms: no samples"); return 1; }
        AVT_HIP(hipSetDevice(tr->device));
        return root_histograms(tr, n_features, hist, minmax);
    });
}

}  // extern "C"
