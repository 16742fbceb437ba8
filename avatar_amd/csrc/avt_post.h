// avt_post.h (private) — the device post-processing of label batches (avt_post.hip): connected components per part on the
// interval grid, the rule of DESIGN.md §8.  One state block per labelling handle (avt_label.h, where the stage's entry points
// are): the scratch of a run, grown on demand, and the centre-of-mass memory of every image slot, which lives across calls.
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
