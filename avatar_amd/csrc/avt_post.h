// avt_post.h (private) — the device post-processing of label batches (avt_post.hip): connected components per part on the
// interval grid, the rule of DESIGN.md §8.  One state block per forest handle (avt_rtree, avt_rforest): the scratch of a run,
// grown on demand, and the centre-of-mass memory of every image slot, which lives across calls.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "avt_host.h"

struct AvtPostState {
    // scratch of one run, n x ceil(rows / interval) x ceil(cols / interval) grid pixels
    DevBuf<int> parent;                      // union-find parent as an index into the image's grid (row stride = grid width of the whole image); -1: background
    DevBuf<int> count;                       // at a root: grid pixels of the component
    DevBuf<unsigned long long> sums;         // at a root: [2 p] sum of the grid columns j, [2 p + 1] of the grid rows i
    DevBuf<unsigned long long> best;         // n x num_parts: bit pattern of the largest score > 0 (0: none)
    DevBuf<int> win;                         // n x num_parts: the winning root (AVT_POST_NONE: none)
    DevBuf<unsigned> status;                 // n: AVT_POST_BAD_LABEL | AVT_POST_FAULT per image
    DevBuf<int> boxes;                       // n x 4: the host boxes of avt_*_post_process_resident
    std::vector<int> h_boxes;                // ... where they wait for the copy
    std::vector<unsigned> h_status;
    // memory across frames: slot s belongs to image s of a batch
    DevBuf<double> com;                      // slots x num_parts x 2 (x, y)
    DevBuf<int> valid;                       // slots: 0 = not sized yet
    int slots = 0;
};

#define AVT_POST_BAD_LABEL 1u                // a label that is neither 255 nor < num_parts: the image is not written
#define AVT_POST_FAULT 2u                    // a bounded union / find loop ran out
#define AVT_POST_NONE 0x7f7f7f7f             // what a byte fill leaves: larger than every grid index (< 2^30)

// Queues the whole stage for n images of rows x cols at d_labels on `stream`; box i is d_boxes[i * box_stride + 0..3]
// (tl.x tl.y br.x br.y, device memory; a box that is empty or not inside the image leaves its labels alone and sets every
// com_pre.x of its slot to -1).  No host wait.  avt_post_finish waits for the stream and turns the status words into a return
// value (0, 1 with a message, or AVT_STATUS_DEVICE_FAULT).
int avt_post_launch(AvtPostState* ps, hipStream_t stream, unsigned char* d_labels, int n, int rows, int cols, const int* d_boxes, int box_stride,
                    int interval, int num_parts, int part_map_type, double dist_to_pre_weight);
int avt_post_finish(AvtPostState* ps, hipStream_t stream, int n, const char* who);
// the slots [first, first + n) of the memory; com is n x num_parts x 2, valid n bytes.  Slots that were never set read as not sized.
int avt_post_com_set(AvtPostState* ps, hipStream_t stream, int num_parts, int first, int n, const double* com, const unsigned char* valid);
int avt_post_com_get(AvtPostState* ps, hipStream_t stream, int num_parts, int first, int n, double* com, unsigned char* valid);

// ---- the two entry points of a forest handle H (avt_rtree, avt_rforest: device, stream, d_labels, n_labels, rows, cols,
// num_parts, part_map_type, post), written once
#include <string>

#include "avt_bgsub_internal.h"

template <class H>
int avt_post_resident(H* h, const char* who, int interval, const int* boxes, double dist_to_pre_weight) {
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

template <class H>
int avt_post_from_bgsub(H* h, avt_bgsub* bg, const char* who, int interval, double dist_to_pre_weight) {
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

// label images that did not come from the handle's own labelling (another classifier, a file, a test): they become the images
// of "the last labelling call"; the handle has no resident depth of its own afterwards
template <class H>
int avt_post_labels_upload(H* h, const char* who, int n, int rows, int cols, const unsigned char* labels) {
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
