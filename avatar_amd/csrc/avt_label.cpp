// avt_label.cpp — the image side of a labelling handle (avt_label.h), once for the tree and the forest: checks, copies and stream
// logic only.  The kernels are the callers' (avt_rtree.hip, avt_rforest.hip, avt_post.hip), the error texts' words come in as
// AvtLabelNames.
#include "avt_label.h"

#include <string>

namespace {

std::string host_only(const AvtLabelNames& k) { return std::string(k.prefix) + ": created host-only (device < 0): inference needs a GPU"; }
std::string fn(const AvtLabelNames& k, const char* rest) { return std::string(k.abi) + rest; }

int batch_ok(const AvtLabelNames& k, int max_images, int n_images) {
    if (max_images && n_images > max_images) { avt_set_error(std::string(k.prefix) + ": at most " + std::to_string(max_images) + " images per call"); return 1; }
    return 0;
}

int reserve_images(AvtLabelHandle* h, const AvtLabelNames& k, size_t pixels) {
    if (h->device < 0) { avt_set_error(host_only(k)); return 1; }
    if (pixels <= h->d_depth.cap && pixels <= h->d_labels.cap) return 0;   // each on its own: a failed allocation leaves that buffer empty
    AVT_HIP(hipSetDevice(h->device));
    return h->d_depth.reserve(pixels) || h->d_labels.reserve(pixels);
}

}  // namespace

int avt_label_roi_ok(const AvtLabelNames& k, int rows, int cols, int interval, int& tlx, int& tly, int& brx, int& bry) {
    if (brx == -1) { brx = cols - 1; bry = rows - 1; }
    if (rows <= 0 || cols <= 0 || interval <= 0 || tlx < 0 || tly < 0 || brx >= cols || bry >= rows || tlx > brx || tly > bry || rows >= 32768 ||
        cols >= 32768) {
        avt_set_error(std::string(k.prefix) + ": bad image size, interval or region of interest");
        return 1;
    }
    return 0;
}

int avt_label_images_upload(AvtLabelHandle* h, const AvtLabelNames& k, int max_images, int n_images, int rows, int cols, const float* depth) {
    if (!h || !depth || n_images <= 0 || rows <= 0 || cols <= 0) { avt_set_error(fn(k, "_images_upload: bad arguments")); return 1; }
    if (batch_ok(k, max_images, n_images)) return 1;
    const size_t pixels = (size_t)n_images * rows * cols;
    if (reserve_images(h, k, pixels)) return 1;
    AVT_HIP(hipSetDevice(h->device));
    AVT_HIP(hipMemcpyAsync(h->d_depth, depth, pixels * sizeof(float), hipMemcpyHostToDevice, h->stream));
    h->n_images = h->n_labels = n_images; h->rows = rows; h->cols = cols;
    return 0;
}

int avt_label_labels_download(AvtLabelHandle* h, const AvtLabelNames& k, int image, unsigned char* out) {
    if (!h || !out || image < 0 || image >= h->n_labels) { avt_set_error(fn(k, "_labels_download: bad arguments")); return 1; }
    const size_t px = (size_t)h->rows * h->cols;
    AVT_HIP(hipMemcpyAsync(out, h->d_labels + px * image, px, hipMemcpyDeviceToHost, h->stream));
    AVT_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

int avt_label_labels_download_all(AvtLabelHandle* h, const AvtLabelNames& k, unsigned char* out) {
    if (!h || !out || h->n_labels <= 0) { avt_set_error(fn(k, "_labels_download_all: bad arguments or no labelled images")); return 1; }
    AVT_HIP(hipMemcpyAsync(out, h->d_labels, (size_t)h->n_labels * h->rows * h->cols, hipMemcpyDeviceToHost, h->stream));
    AVT_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

int avt_label_predict_resident_boxes(AvtLabelHandle* h, const AvtLabelNames& k, int interval, const int* boxes, int fill, AvtLabelLaunchBoxes launch) {
    if (!h || !boxes) { avt_set_error(fn(k, "_predict_best_resident_boxes: null argument")); return 1; }
    if (h->device < 0) { avt_set_error(host_only(k)); return 1; }
    if (h->n_images <= 0) { avt_set_error(fn(k, "_predict_best_resident_boxes: no images resident")); return 1; }
    const int n = h->n_images, rows = h->rows, cols = h->cols;
    // everything is checked before anything is queued: after a failure the labels of the previous call are still there
    std::vector<int> b(boxes, boxes + 4 * (size_t)n);
    for (int i = 0; i < n; ++i) {
        int* q = &b[4 * (size_t)i];
        if (q[2] == -1) { q[2] = cols - 1; q[3] = rows - 1; }
        if (q[0] > q[2] || q[1] > q[3]) continue;          // an empty box: that image stays 255 (a lost stream does not fail the batch)
        if (avt_label_roi_ok(k, rows, cols, interval, q[0], q[1], q[2], q[3])) return 1;
    }
    int tlx = 0, tly = 0, brx = -1, bry = -1;
    if (avt_label_roi_ok(k, rows, cols, interval, tlx, tly, brx, bry)) return 1;     // the interval and the image size, when every box is empty
    AVT_HIP(hipSetDevice(h->device));
    if (h->d_boxes.reserve(4 * (size_t)n)) return 1;
    AVT_HIP(hipMemcpyAsync(h->d_boxes, b.data(), b.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    AVT_HIP(hipStreamSynchronize(h->stream));              // `b` is on this stack frame
    if (launch(h, h->d_depth, h->d_boxes, 4, n, rows, cols, interval, fill)) { avt_set_error(std::string(k.prefix) + ": kernel launch failed"); return 1; }
    return 0;
}

int avt_label_predict_from_bgsub(AvtLabelHandle* h, const AvtLabelNames& k, int max_images, avt_bgsub* bg, int interval, int fill, AvtLabelLaunchBoxes launch) {
    if (!h) { avt_set_error(fn(k, "_predict_best_from_bgsub: null ") + k.noun); return 1; }
    if (h->device < 0) { avt_set_error(host_only(k)); return 1; }
    if (!bg) { avt_set_error(fn(k, "_predict_best_from_bgsub: null background subtractor")); return 1; }
    avt_bgsub_view v;
    if (avt_bgsub_last_run(bg, &v)) return 1;
    if (v.device != h->device) {
        avt_set_error(fn(k, "_predict_best_from_bgsub: the ") + k.noun + " and the background subtractor are on different devices");
        return 1;
    }
    int tlx = 0, tly = 0, brx = -1, bry = -1;
    if (avt_label_roi_ok(k, v.rows, v.cols, interval, tlx, tly, brx, bry) || batch_ok(k, max_images, v.n_images)) return 1;
    AVT_HIP(hipSetDevice(h->device));
    const size_t pixels = (size_t)v.n_images * v.rows * v.cols;
    if (h->d_labels.reserve(pixels)) return 1;
    // the labels are these images' from here on, and the handle has no resident depth of its own until the next images_upload
    h->n_images = 0; h->n_labels = v.n_images; h->rows = v.rows; h->cols = v.cols;
    // the handle's stream waits for the run; bg's next upload / run / destroy waits for the labelling.  No copy, no host wait.
    if (avt_bgsub_reader_begin(bg, h->stream)) return 1;
    const int rc = launch(h, v.d_depth, v.d_boxes, v.box_stride, v.n_images, v.rows, v.cols, interval, fill);
    if (avt_bgsub_reader_end(bg, h->stream)) return 1;     // also after a failed launch: the memset may be queued
    if (rc) { avt_set_error(std::string(k.prefix) + ": kernel launch failed"); return 1; }
    return 0;
}

int avt_label_predict_dist(AvtLabelHandle* h, const AvtLabelNames& k, bool side_limit, const float* depth, int rows, int cols, float* dist_out,
                           AvtLabelLaunchDist launch) {
    if (!h || !depth || !dist_out || rows <= 0 || cols <= 0) { avt_set_error(fn(k, "_predict: bad arguments")); return 1; }
    if (side_limit && (rows >= 32768 || cols >= 32768)) { avt_set_error(std::string(k.prefix) + ": bad image size, interval or region of interest"); return 1; }
    if (avt_label_images_upload(h, k, 0, 1, rows, cols, depth)) return 1;
    const size_t n = (size_t)h->num_parts * rows * cols;
    DevBuf<float> d_out;
    if (d_out.reserve(n)) return 1;
    int rc = launch(h, rows, cols, d_out);
    if (rc) avt_set_error(std::string(k.prefix) + ": kernel launch failed");
    if (!rc && hipMemcpyAsync(dist_out, d_out, n * sizeof(float), hipMemcpyDeviceToHost, h->stream) != hipSuccess) {
        avt_set_error(std::string(k.prefix) + ": download failed");
        rc = 1;
    }
    if (hipStreamSynchronize(h->stream) != hipSuccess && !rc) { avt_set_error(std::string(k.prefix) + ": stream failed"); rc = 1; }   // on every path, before d_out goes
    return rc;
}

int avt_label_sync(AvtLabelHandle* h, const AvtLabelNames& k, bool refuse_host_only) {
    if (!h) { avt_set_error(fn(k, "_sync: null ") + k.noun); return 1; }
    if (refuse_host_only && h->device < 0) { avt_set_error(host_only(k)); return 1; }
    AVT_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

void avt_label_teardown(AvtLabelHandle* h) {
    // the buffers go with `delete`, after the stream: it is drained first, so nothing is queued on them either way
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    h->stream = nullptr;
}

int avt_label_com_pre_set(AvtLabelHandle* h, const AvtLabelNames& k, int first, int n, const double* com, const unsigned char* valid) {
    if (!h || h->device < 0) { avt_set_error(fn(k, "_com_pre_set: null or host-only ") + k.noun); return 1; }
    AVT_HIP(hipSetDevice(h->device));
    return avt_post_com_set(&h->post, h->stream, h->num_parts, first, n, com, valid);
}

int avt_label_com_pre_get(AvtLabelHandle* h, const AvtLabelNames& k, int first, int n, double* com, unsigned char* valid) {
    if (!h || h->device < 0) { avt_set_error(fn(k, "_com_pre_get: null or host-only ") + k.noun); return 1; }
    AVT_HIP(hipSetDevice(h->device));
    return avt_post_com_get(&h->post, h->stream, h->num_parts, first, n, com, valid);
}

// ---- the device post-processing behind a handle
int avt_post_resident(AvtLabelHandle* h, const char* who, int interval, const int* boxes, double dist_to_pre_weight) {
    if (!h) { avt_set_error(std::string(who) + ": null handle"); return 1; }
    if (h->device < 0) { avt_set_error(std::string(who) + ": created host-only (device < 0): the device stage needs a GPU"); return 1; }
    if (h->n_labels <= 0) { avt_set_error(std::string(who) + ": no labelled images behind the handle"); return 1; }
    const int n = h->n_labels, rows = h->rows, cols = h->cols;
    if (interval <= 0) { avt_set_error(std::string(who) + ": bad interval"); return 1; }
    // everything is checked before anything is queued: after a failure labels and memory are as they were
    std::vector<int>& b = h->post.h_boxes;             // lives until the copy has been waited for (avt_post_finish)
    b.assign(4 * (size_t)n, 0);
    for (int i = 0; i < n; ++i) {
        int* q = &b[4 * (size_t)i];
        if (boxes) for (int k = 0; k < 4; ++k) q[k] = boxes[4 * (size_t)i + k];
        else q[2] = -1;
        if (q[2] == -1) { q[2] = cols - 1; q[3] = rows - 1; }
        if (q[0] > q[2] || q[1] > q[3]) continue;      // an empty box (a lost stream): labels untouched, every com_pre.x -1
        if (q[0] < 0 || q[1] < 0 || q[2] >= cols || q[3] >= rows) { avt_set_error(std::string(who) + ": bad region of interest"); return 1; }
    }
    AVT_HIP(hipSetDevice(h->device));
    if (h->post.boxes.reserve(4 * (size_t)n)) return 1;
    AVT_HIP(hipMemcpyAsync(h->post.boxes, b.data(), b.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    if (avt_post_launch(&h->post, h->stream, h->d_labels, n, rows, cols, h->post.boxes, 4, interval, h->num_parts, h->part_map_type, dist_to_pre_weight)) {
        (void)hipStreamSynchronize(h->stream);
        return 1;
    }
    return avt_post_finish(&h->post, h->stream, n, who);
}

int avt_post_from_bgsub(AvtLabelHandle* h, avt_bgsub* bg, const char* who, int interval, double dist_to_pre_weight) {
    if (!h) { avt_set_error(std::string(who) + ": null handle"); return 1; }
    if (h->device < 0) { avt_set_error(std::string(who) + ": created host-only (device < 0): the device stage needs a GPU"); return 1; }
    if (!bg) { avt_set_error(std::string(who) + ": null background subtractor"); return 1; }
    avt_bgsub_view v;
    if (avt_bgsub_last_run(bg, &v)) return 1;
    if (v.device != h->device) { avt_set_error(std::string(who) + ": the handle and the background subtractor are on different devices"); return 1; }
    if (h->n_labels != v.n_images || h->rows != v.rows || h->cols != v.cols) {
        avt_set_error(std::string(who) + ": the labels behind the handle are not those of the background subtractor's last run");
        return 1;
    }
    if (interval <= 0) { avt_set_error(std::string(who) + ": bad interval"); return 1; }
    AVT_HIP(hipSetDevice(h->device));
    // the handle's stream waits for the run; bg's next upload / run / destroy waits for this stage, as for the labelling
    if (avt_bgsub_reader_begin(bg, h->stream)) return 1;
    const int rc = avt_post_launch(&h->post, h->stream, h->d_labels, v.n_images, v.rows, v.cols, v.d_boxes, v.box_stride, interval, h->num_parts,
                                   h->part_map_type, dist_to_pre_weight);
    if (avt_bgsub_reader_end(bg, h->stream)) return 1;
    if (rc) { (void)hipStreamSynchronize(h->stream); return 1; }
    return avt_post_finish(&h->post, h->stream, v.n_images, who);
}

int avt_post_labels_upload(AvtLabelHandle* h, const char* who, int n, int rows, int cols, const unsigned char* labels) {
    if (!h || !labels || n <= 0 || n > 65535 || rows <= 0 || cols <= 0 || rows >= 32768 || cols >= 32768) {
        avt_set_error(std::string(who) + ": bad arguments (1 to 65535 images of 1 to 32767 rows and columns)");
        return 1;
    }
    if (h->device < 0) { avt_set_error(std::string(who) + ": created host-only (device < 0): the device stage needs a GPU"); return 1; }
    AVT_HIP(hipSetDevice(h->device));
    const size_t bytes = (size_t)n * rows * cols;
    AVT_HIP(hipStreamSynchronize(h->stream));          // nothing queued still reads the labels that reserve() may free
    if (h->d_labels.reserve(bytes)) return 1;
    AVT_HIP(hipMemcpyAsync(h->d_labels, labels, bytes, hipMemcpyHostToDevice, h->stream));
    AVT_HIP(hipStreamSynchronize(h->stream));          // the caller's buffer is free on return
    h->n_images = 0; h->n_labels = n; h->rows = rows; h->cols = cols;
    return 0;
}
