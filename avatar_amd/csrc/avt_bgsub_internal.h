// avt_bgsub_internal.h (private) — what another stage of libavatar_hip.so needs to read the result of the last
// avt_bgsub_run_resident where it lies on the device (avt_rtree_predict_best_from_bgsub).  Not part of the public bgsub ABI.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/avt_bgsub.h"

struct avt_bgsub_view {
    int device, n_images, rows, cols;
    const float* d_depth;        // n_images x rows x cols masked depth
    const int* d_boxes;          // image i's box (tl.x tl.y br.x br.y) at d_boxes[i * box_stride]
    int box_stride;              // in ints
    const float* d_xyz;          // n_images x rows x cols x 3: the XYZ maps as uploaded (or back-projected); no run masks them
};

// The last run's result; fails ("no run") when no avt_bgsub_run_resident followed the last upload.
int avt_bgsub_last_run(avt_bgsub* bg, avt_bgsub_view* out);
// The resident images whether or not a run followed their upload: d_xyz is valid, d_depth and the boxes only when *ran.
// Fails ("no images resident") before the first upload.
int avt_bgsub_resident(avt_bgsub* bg, avt_bgsub_view* out, bool* ran);
// A reader on another stream of the same device brackets its work with these two.  begin: `reader` waits for everything
// queued on bg's stream so far (the run).  end: bg's next images_upload, run_resident and destroy wait for everything queued
// on `reader` so far.  No host synchronisation in either.
int avt_bgsub_reader_begin(avt_bgsub* bg, hipStream_t reader);
int avt_bgsub_reader_end(avt_bgsub* bg, hipStream_t reader);
