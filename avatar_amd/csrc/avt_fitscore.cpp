// avt_fitscore.cpp — host side of the fit score (include/avt_fitscore.h): argument checks, the staging of host images in bounded
// batches, the hand-over from the renderer and from the background subtractor, and the one wait at the end of a call that
// brings the tables and the bad-label flag back.
#include "avt_fitscore.h"

#include <algorithm>
#include <cmath>
#include <string>

#include "avt_bgsub_internal.h"
#include "avt_internal.h"
#include "avt_rtree_train.h"

namespace {

const char* const kHostOnly = "fitscore: created host-only (device < 0): scoring needs a GPU";
const size_t kStageBytes = (size_t)256 << 20;     // host images are staged this many bytes at a time (9 per pixel)

size_t cells_of(const avt_fitscore* fs) { return (size_t)(fs->num_parts + 1) * AVT_FITSCORE_COLS; }

int create_impl(int device, int num_parts, int max_images, avt_fitscore** out) {
    if (!out) { avt_set_error("avt_fitscore_create: null argument"); return 1; }
    if (num_parts < 1 || num_parts > 254) { avt_set_error("avt_fitscore_create: num_parts " + std::to_string(num_parts) + ": a scorer has 1 to 254 parts"); return 1; }
    if (max_images < 1) { avt_set_error("avt_fitscore_create: needs max_images >= 1"); return 1; }
    avt_fitscore* fs = new avt_fitscore();
    fs->device = device; fs->num_parts = num_parts; fs->max_images = max_images;
    auto on_device = [&]() -> int {
        if (device < 0) return 0;
        AVT_HIP(hipSetDevice(device));
        AVT_HIP(hipStreamCreateWithFlags(&fs->stream, hipStreamNonBlocking));
        return fs->d_table.reserve(cells_of(fs) * max_images) || fs->d_bad.reserve(1) || fs->d_boxes.reserve(4 * (size_t)max_images) ||
               fs->d_index.reserve((size_t)max_images);
    };
    if (on_device()) { avt_fitscore_destroy(fs); return 1; }
    *out = fs;
    return 0;
}

// the checks every scoring call shares, before anything is queued; the handle holds no result from here until commit()
int call_ok(avt_fitscore* fs, const std::string& who, float tol, int stride) {
    if (!fs) { avt_set_error(who + ": null scorer"); return 1; }
    fs->n_result = 0;
    if (!(tol >= 0.f)) { avt_set_error(who + ": tol must be >= 0 (+inf allowed), not negative or NaN"); return 1; }
    if (stride < 1) { avt_set_error(who + ": needs stride >= 1"); return 1; }
    return 0;
}

int size_ok(avt_fitscore* fs, const std::string& who, int n, int rows, int cols) {
    if (n < 1 || rows < 1 || cols < 1 || rows >= 32768 || cols >= 32768) {
        avt_set_error(who + ": needs n_images >= 1 and images of 1 to 32767 rows and columns");
        return 1;
    }
    if (n > fs->max_images) { avt_set_error(who + ": " + std::to_string(n) + " images, the scorer was created for " + std::to_string(fs->max_images)); return 1; }
    return 0;
}

int begin(avt_fitscore* fs, int n) {
    AVT_HIP(hipMemsetAsync(fs->d_table, 0, cells_of(fs) * n * sizeof(unsigned long long), fs->stream));
    AVT_HIP(hipMemsetAsync(fs->d_bad, 0, sizeof(int), fs->stream));
    return 0;
}

// the call's one host wait (also the contract of avt_renderer_images_for): the tables and the flag come back behind the kernels
int commit(avt_fitscore* fs, const std::string& who, int n) {
    int bad = 0;
    fs->table.resize(cells_of(fs) * n);
    AVT_HIP(hipMemcpyAsync(fs->table.data(), fs->d_table, fs->table.size() * sizeof(long long), hipMemcpyDeviceToHost, fs->stream));
    AVT_HIP(hipMemcpyAsync(&bad, fs->d_bad, sizeof(int), hipMemcpyDeviceToHost, fs->stream));
    AVT_HIP(hipStreamSynchronize(fs->stream));
    if (bad) {
        avt_set_error(who + ": a part-mask label at a selected pixel is >= num_parts (" + std::to_string(fs->num_parts) + ") and not 255; the call holds no result");
        return 1;
    }
    fs->n_result = n;
    return 0;
}

int images_impl(avt_fitscore* fs, int n, int rows, int cols, const float* model, const unsigned char* mask, const float* obs, const int* boxes,
                float tol, int stride) {
    const std::string who = "avt_fitscore_images";
    if (call_ok(fs, who, tol, stride)) return 1;
    if (!model || !mask || !obs) { avt_set_error(who + ": null argument"); return 1; }
    if (size_ok(fs, who, n, rows, cols)) return 1;
    if (fs->device < 0) { avt_set_error(kHostOnly); return 1; }
    AVT_HIP(hipSetDevice(fs->device));
    const size_t npix = (size_t)rows * cols;
    const int batch = (int)std::max<size_t>(1, std::min<size_t>(n, kStageBytes / (npix * 9)));
    auto fail = [&](bool set) { if (set) avt_set_error(who + ": device call failed"); (void)hipStreamSynchronize(fs->stream); return 1; };
    if (fs->d_model.reserve(batch * npix) || fs->d_obs.reserve(batch * npix) || fs->d_mask.reserve(batch * npix) || begin(fs, n)) return fail(false);
    if (boxes && hipMemcpyAsync(fs->d_boxes, boxes, 4 * (size_t)n * sizeof(int), hipMemcpyHostToDevice, fs->stream) != hipSuccess) return fail(true);
    for (int i0 = 0; i0 < n; i0 += batch) {
        const int k = std::min(batch, n - i0);
        const FitScoreJob job{fs->d_model, fs->d_mask, fs->d_obs, boxes ? fs->d_boxes + 4 * (size_t)i0 : nullptr, 4, nullptr, k, rows, cols, stride, tol};
        if (hipMemcpyAsync(fs->d_model, model + i0 * npix, k * npix * sizeof(float), hipMemcpyHostToDevice, fs->stream) != hipSuccess ||
            hipMemcpyAsync(fs->d_mask, mask + i0 * npix, k * npix, hipMemcpyHostToDevice, fs->stream) != hipSuccess ||
            hipMemcpyAsync(fs->d_obs, obs + i0 * npix, k * npix * sizeof(float), hipMemcpyHostToDevice, fs->stream) != hipSuccess ||
            avt_fitscore_launch(fs, job, fs->d_table + cells_of(fs) * i0, fs->d_bad) ||
            (i0 + k < n && hipStreamSynchronize(fs->stream) != hipSuccess))      // the next batch goes into the same buffers
            return fail(true);
    }
    return commit(fs, who, n);
}

// the model side of the two renderer forms: from here fs->stream waits for the renderer, and every path of the caller drains it
// before it returns, as avt_renderer_images_for asks
int model_side(avt_fitscore* fs, const std::string& who, avt_renderer* r, const float** depth, const unsigned char** mask, int* n, int* w, int* h) {
    if (avt_renderer_images_for(r, fs->stream, depth, mask, n, w, h)) return 1;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, *depth) != hipSuccess || at.device != fs->device) {
        (void)hipGetLastError();
        avt_set_error(who + ": the scorer and the renderer are on different devices");
        return 2;
    }
    if (hipSetDevice(fs->device) != hipSuccess) { avt_set_error(who + ": hipSetDevice failed"); return 2; }
    return size_ok(fs, who, *n, *h, *w) ? 2 : 0;
}

int rendered_impl(avt_fitscore* fs, avt_renderer* r, const float* obs, const int* boxes, float tol, int stride) {
    const std::string who = "avt_fitscore_rendered";
    if (call_ok(fs, who, tol, stride)) return 1;
    if (!obs) { avt_set_error(who + ": null argument"); return 1; }
    if (fs->device < 0) { avt_set_error(kHostOnly); return 1; }
    if (!r) { avt_set_error(who + ": null renderer"); return 1; }
    const float* depth = nullptr;
    const unsigned char* mask = nullptr;
    int n = 0, w = 0, h = 0;
    const int ms = model_side(fs, who, r, &depth, &mask, &n, &w, &h);
    if (ms == 1) return 1;
    auto drain = [&]() { (void)hipStreamSynchronize(fs->stream); return 1; };
    if (ms) return drain();
    const size_t pixels = (size_t)n * h * w;
    if (fs->d_obs.reserve(pixels) || begin(fs, n)) return drain();
    const FitScoreJob job{depth, mask, fs->d_obs, boxes ? (const int*)fs->d_boxes : nullptr, 4, nullptr, n, h, w, stride, tol};
    if ((boxes && hipMemcpyAsync(fs->d_boxes, boxes, 4 * (size_t)n * sizeof(int), hipMemcpyHostToDevice, fs->stream) != hipSuccess) ||
        hipMemcpyAsync(fs->d_obs, obs, pixels * sizeof(float), hipMemcpyHostToDevice, fs->stream) != hipSuccess ||
        avt_fitscore_launch(fs, job, fs->d_table, fs->d_bad)) {
        avt_set_error(who + ": device call failed");
        return drain();
    }
    return commit(fs, who, n);
}

int from_bgsub_impl(avt_fitscore* fs, avt_renderer* r, avt_bgsub* bg, const int* obs_index, float tol, int stride) {
    const std::string who = "avt_fitscore_rendered_from_bgsub";
    if (call_ok(fs, who, tol, stride)) return 1;
    if (fs->device < 0) { avt_set_error(kHostOnly); return 1; }
    if (!r) { avt_set_error(who + ": null renderer"); return 1; }
    if (!bg) { avt_set_error(who + ": null background subtractor"); return 1; }
    avt_bgsub_view v;
    if (avt_bgsub_last_run(bg, &v)) return 1;
    if (v.device != fs->device) { avt_set_error(who + ": the scorer and the background subtractor are on different devices"); return 1; }
    const float* depth = nullptr;
    const unsigned char* mask = nullptr;
    int n = 0, w = 0, h = 0;
    const int ms = model_side(fs, who, r, &depth, &mask, &n, &w, &h);
    if (ms == 1) return 1;
    auto drain = [&]() { (void)hipStreamSynchronize(fs->stream); return 1; };
    if (ms) return drain();
    if (h != v.rows || w != v.cols) {
        avt_set_error(who + ": the renderer's images are " + std::to_string(w) + " x " + std::to_string(h) + ", the background subtractor's " +
                      std::to_string(v.cols) + " x " + std::to_string(v.rows));
        return drain();
    }
    if (!obs_index && n > v.n_images) {
        avt_set_error(who + ": " + std::to_string(n) + " rendered images for " + std::to_string(v.n_images) + " observed ones");
        return drain();
    }
    for (int i = 0; obs_index && i < n; ++i)
        if (obs_index[i] < 0 || obs_index[i] >= v.n_images) {
            avt_set_error(who + ": obs_index[" + std::to_string(i) + "] = " + std::to_string(obs_index[i]) + ": the last run holds " + std::to_string(v.n_images) + " images");
            return drain();
        }
    // the scorer's stream waits for the run; bg's next upload / run / destroy waits for the scoring.  No copy of an image.
    if (avt_bgsub_reader_begin(bg, fs->stream)) return drain();
    const FitScoreJob job{depth, mask, v.d_depth, v.d_boxes, v.box_stride, obs_index ? (const int*)fs->d_index : nullptr, n, h, w, stride, tol};
    const bool failed = begin(fs, n) ||
                        (obs_index && hipMemcpyAsync(fs->d_index, obs_index, (size_t)n * sizeof(int), hipMemcpyHostToDevice, fs->stream) != hipSuccess) ||
                        avt_fitscore_launch(fs, job, fs->d_table, fs->d_bad);
    if (avt_bgsub_reader_end(bg, fs->stream)) return drain();      // also after a failed launch: the memsets may be queued
    if (failed) { avt_set_error(who + ": device call failed"); return drain(); }
    return commit(fs, who, n);
}

int get_impl(avt_fitscore* fs, long long* table, int* n_images) {
    if (!fs) { avt_set_error("avt_fitscore_get: null scorer"); return 1; }
    if (fs->n_result <= 0) { avt_set_error("avt_fitscore_get: no score (no scoring call succeeded since the handle was created, or the last one failed)"); return 1; }
    if (table) std::copy(fs->table.begin(), fs->table.begin() + cells_of(fs) * fs->n_result, table);
    if (n_images) *n_images = fs->n_result;
    return 0;
}

}  // namespace

// ---- exported entry points: no C++ exception crosses the C ABI
extern "C" {

int avt_fitscore_create(int device, int num_parts, int max_images, avt_fitscore** out) {
    return avt_guard("avt_fitscore_create", [&]() -> int { return create_impl(device, num_parts, max_images, out); });
}

void avt_fitscore_destroy(avt_fitscore* fs) {
    if (!fs) return;
    // the buffers go with `delete`, after the stream: it is drained first, so nothing is queued on them either way
    if (fs->stream) (void)hipStreamSynchronize(fs->stream);
    if (fs->stream) (void)hipStreamDestroy(fs->stream);
    delete fs;
}

int avt_fitscore_images(avt_fitscore* fs, int n_images, int rows, int cols, const float* model_depth, const unsigned char* model_mask,
                        const float* observed, const int* boxes, float tol, int stride) {
    return avt_guard("avt_fitscore_images", [&]() -> int { return images_impl(fs, n_images, rows, cols, model_depth, model_mask, observed, boxes, tol, stride); });
}

int avt_fitscore_rendered(avt_fitscore* fs, struct avt_renderer* r, const float* observed, const int* boxes, float tol, int stride) {
    return avt_guard("avt_fitscore_rendered", [&]() -> int { return rendered_impl(fs, r, observed, boxes, tol, stride); });
}

int avt_fitscore_rendered_from_bgsub(avt_fitscore* fs, struct avt_renderer* r, struct avt_bgsub* bg, const int* obs_index, float tol, int stride) {
    return avt_guard("avt_fitscore_rendered_from_bgsub", [&]() -> int { return from_bgsub_impl(fs, r, bg, obs_index, tol, stride); });
}

int avt_fitscore_get(avt_fitscore* fs, long long* table, int* n_images) {
    return avt_guard("avt_fitscore_get", [&]() -> int { return get_impl(fs, table, n_images); });
}

int avt_fitscore_sync(avt_fitscore* fs) {
    if (!fs) { avt_set_error("avt_fitscore_sync: null scorer"); return 1; }
    if (fs->device < 0) { avt_set_error(kHostOnly); return 1; }
    AVT_HIP(hipStreamSynchronize(fs->stream));
    return 0;
}

}  // extern "C"
