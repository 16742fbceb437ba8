// avt_poseerr.cpp — host side of the pose error (include/avt_poseerr.h): argument checks, the part-sorted vertex list built at
// creation, the two ways a side's points arrive (from the host, from a context on the device) and the one wait of a get.
#include "avt_poseerr.h"

#include <algorithm>
#include <string>

#include "avt_internal.h"

namespace {

const char* const kHostOnly = "poseerr: created host-only (device < 0): scoring needs a GPU";

int create_impl(int device, int V, int J, int P, const int* vertex_part, int max_pairs, avt_poseerr** out) {
    const std::string who = "avt_poseerr_create";
    if (!out) { avt_set_error(who + ": null argument"); return 1; }
    if (V < 1 || J < 0 || V >= (1 << 28) || J >= (1 << 28)) { avt_set_error(who + ": needs V >= 1 vertices and J >= 0 joints"); return 1; }
    if (P < 1 || P > 254) { avt_set_error(who + ": num_parts " + std::to_string(P) + ": a scorer has 1 to 254 parts"); return 1; }
    if (!vertex_part && P != 1) { avt_set_error(who + ": a null vertex_part puts every vertex in part 0 and needs num_parts == 1"); return 1; }
    if (max_pairs < 1) { avt_set_error(who + ": needs max_pairs >= 1"); return 1; }
    std::vector<int> pstart((size_t)P + 1, 0), perm((size_t)V);
    for (int v = 0; v < V; ++v) {
        const int q = vertex_part ? vertex_part[v] : 0;
        if (q < 0 || q >= P) {
            avt_set_error(who + ": vertex_part[" + std::to_string(v) + "] = " + std::to_string(q) + " is not in [0, num_parts = " + std::to_string(P) + ")");
            return 1;
        }
        ++pstart[(size_t)q + 1];
    }
    avt_poseerr* pe = new avt_poseerr();
    pe->device = device; pe->V = V; pe->J = J; pe->P = P; pe->max_pairs = max_pairs;
    pe->part_size.assign(pstart.begin() + 1, pstart.end());
    for (int q = 0; q < P; ++q) pstart[(size_t)q + 1] += pstart[(size_t)q];
    {
        std::vector<int> fill(pstart.begin(), pstart.end() - 1);            // counting sort: ascending v inside a part
        for (int v = 0; v < V; ++v) perm[(size_t)fill[(size_t)(vertex_part ? vertex_part[v] : 0)]++] = v;
    }
    auto on_device = [&]() -> int {
        if (device < 0) return 0;
        AVT_HIP(hipSetDevice(device));
        AVT_HIP(hipStreamCreateWithFlags(&pe->stream, hipStreamNonBlocking));
        AVT_HIP(hipEventCreateWithFlags(&pe->ev_in, hipEventDisableTiming));
        AVT_HIP(hipEventCreateWithFlags(&pe->ev_out, hipEventDisableTiming));
        const size_t n = (size_t)max_pairs, j = (size_t)std::max(J, 1);
        if (pe->d_perm.reserve((size_t)V) || pe->d_pstart.reserve((size_t)P + 1) || pe->d_dist.reserve(n * V) ||
            pe->d_summary.reserve(n * AVT_POSEERR_COLS) || pe->d_per_joint.reserve(n * 2 * j) || pe->d_per_part.reserve(n * 2 * P) ||
            pe->d_argmax.reserve(n * 2) || pe->d_status.reserve(n))
            return 1;
        for (int s = 0; s < 2; ++s)
            if (pe->d_cloud[s].reserve(n * 3 * V) || pe->d_joints[s].reserve(n * 3 * j)) return 1;
        AVT_HIP(hipMemcpyAsync(pe->d_perm, perm.data(), (size_t)V * sizeof(int), hipMemcpyHostToDevice, pe->stream));
        AVT_HIP(hipMemcpyAsync(pe->d_pstart, pstart.data(), ((size_t)P + 1) * sizeof(int), hipMemcpyHostToDevice, pe->stream));
        AVT_HIP(hipStreamSynchronize(pe->stream));                          // the host tables are on this stack frame
        return 0;
    };
    if (on_device()) { avt_poseerr_destroy(pe); return 1; }
    *out = pe;
    return 0;
}

int create_for_model_impl(int device, const avt_model* m, int P, const int* part_map, int max_pairs, avt_poseerr** out) {
    if (!m || !out) { avt_set_error("avt_poseerr_create_for_model: null argument"); return 1; }
    const int V = m->d.V, J = m->d.J;
    std::vector<int> vp((size_t)std::max(V, 0));
    for (int v = 0; v < V; ++v) {
        const int j = m->main_joint[(size_t)v];
        vp[(size_t)v] = part_map && j >= 0 && j < J ? part_map[j] : j;
    }
    return create_impl(device, V, J, P, vp.data(), max_pairs, out);
}

// the checks upload and from_ctx share
int side_ok(avt_poseerr* pe, const std::string& who, int side, int n) {
    if (!pe) { avt_set_error(who + ": null scorer"); return 1; }
    if (side != AVT_POSEERR_ESTIMATE && side != AVT_POSEERR_TRUTH) { avt_set_error(who + ": side must be AVT_POSEERR_ESTIMATE or AVT_POSEERR_TRUTH"); return 1; }
    if (n < 1) { avt_set_error(who + ": needs n >= 1 pairs"); return 1; }
    if (n > pe->max_pairs) { avt_set_error(who + ": " + std::to_string(n) + " pairs, the scorer was created for " + std::to_string(pe->max_pairs)); return 1; }
    return 0;
}

int upload_impl(avt_poseerr* pe, int side, int n, const double* clouds, const double* joints) {
    const std::string who = "avt_poseerr_upload";
    if (side_ok(pe, who, side, n)) return 1;
    if (!clouds || (!joints && pe->J > 0)) { avt_set_error(who + ": null argument (joints may be null only if J == 0)"); return 1; }
    if (pe->device < 0) { pe->n_side[side] = n; return 0; }                 // host-only: the count is all there is to keep
    pe->n_side[side] = 0;
    AVT_HIP(hipSetDevice(pe->device));
    AVT_HIP(hipMemcpyAsync(pe->d_cloud[side], clouds, (size_t)n * 3 * pe->V * sizeof(double), hipMemcpyHostToDevice, pe->stream));
    if (pe->J > 0) AVT_HIP(hipMemcpyAsync(pe->d_joints[side], joints, (size_t)n * 3 * pe->J * sizeof(double), hipMemcpyHostToDevice, pe->stream));
    AVT_HIP(hipStreamSynchronize(pe->stream));                              // the caller's arrays are free again
    pe->n_side[side] = n;
    return 0;
}

int from_ctx_impl(avt_poseerr* pe, int side, avt_ctx* c, int n, const int* frames) {
    const std::string who = "avt_poseerr_from_ctx";
    if (side_ok(pe, who, side, n)) return 1;
    if (!c) { avt_set_error(who + ": null context"); return 1; }
    if (pe->device < 0) { avt_set_error(kHostOnly); return 1; }
    if (c->dm.d.V != pe->V || c->dm.d.J != pe->J || c->device != pe->device) {
        avt_set_error(who + ": the context's V, J or device is not the scorer's");
        return 1;
    }
    for (int i = 0; i < n; ++i) {
        const int f = frames ? frames[i] : i;
        if (f < 0 || f >= c->fb.max_frames) { avt_set_error(who + ": frame index " + std::to_string(f) + " out of range"); return 1; }
    }
    pe->n_side[side] = 0;
    AVT_HIP(hipSetDevice(pe->device));
    // after everything queued on the context (its side streams join its main stream), and before anything queued on it later
    AVT_HIP(hipEventRecord(pe->ev_in, c->stream));
    AVT_HIP(hipStreamWaitEvent(pe->stream, pe->ev_in, 0));
    const size_t V3 = (size_t)3 * pe->V, J3 = (size_t)3 * pe->J;
    for (int i = 0; i < n;) {
        const int f = frames ? frames[i] : i;
        int run = 1;                                                        // consecutive frames go in one copy
        while (i + run < n && (frames ? frames[i + run] : i + run) == f + run) ++run;
        AVT_HIP(hipMemcpyAsync(pe->d_cloud[side] + (size_t)i * V3, c->fb.cloud + (size_t)f * V3, run * V3 * sizeof(double), hipMemcpyDeviceToDevice, pe->stream));
        if (pe->J > 0)
            AVT_HIP(hipMemcpyAsync(pe->d_joints[side] + (size_t)i * J3, c->fb.jointpos + (size_t)f * J3, run * J3 * sizeof(double), hipMemcpyDeviceToDevice, pe->stream));
        i += run;
    }
    AVT_HIP(hipEventRecord(pe->ev_out, pe->stream));
    AVT_HIP(hipStreamWaitEvent(c->stream, pe->ev_out, 0));
    pe->n_side[side] = n;
    return 0;
}

int run_impl(avt_poseerr* pe) {
    const std::string who = "avt_poseerr_run";
    if (!pe) { avt_set_error(who + ": null scorer"); return 1; }
    pe->n_result = 0;
    const int n = pe->n_side[AVT_POSEERR_ESTIMATE];
    if (n != pe->n_side[AVT_POSEERR_TRUTH]) {
        avt_set_error(who + ": the estimate side holds " + std::to_string(n) + " pairs, the truth side " + std::to_string(pe->n_side[AVT_POSEERR_TRUTH]));
        return 1;
    }
    if (n < 1) { avt_set_error(who + ": no pairs resident (upload or from_ctx both sides first)"); return 1; }
    if (pe->device < 0) { avt_set_error(kHostOnly); return 1; }
    AVT_HIP(hipSetDevice(pe->device));
    if (avt_poseerr_launch(pe, n)) { avt_set_error(who + ": launch failed"); return 1; }
    pe->n_result = n;
    return 0;
}

int get_impl(avt_poseerr* pe, double* summary, double* per_joint, double* per_part, int* argmax, unsigned* status, int* n_out) {
    const std::string who = "avt_poseerr_get";
    if (!pe) { avt_set_error(who + ": null scorer"); return 1; }
    if (pe->n_result <= 0) { avt_set_error(who + ": no result (no run succeeded since the handle was created, or the last one failed)"); return 1; }
    const size_t n = (size_t)pe->n_result;
    AVT_HIP(hipSetDevice(pe->device));
    if (summary) AVT_HIP(hipMemcpyAsync(summary, pe->d_summary, n * AVT_POSEERR_COLS * sizeof(double), hipMemcpyDeviceToHost, pe->stream));
    if (per_joint && pe->J > 0) AVT_HIP(hipMemcpyAsync(per_joint, pe->d_per_joint, n * 2 * pe->J * sizeof(double), hipMemcpyDeviceToHost, pe->stream));
    if (per_part) AVT_HIP(hipMemcpyAsync(per_part, pe->d_per_part, n * 2 * pe->P * sizeof(double), hipMemcpyDeviceToHost, pe->stream));
    if (argmax) AVT_HIP(hipMemcpyAsync(argmax, pe->d_argmax, n * 2 * sizeof(int), hipMemcpyDeviceToHost, pe->stream));
    if (status) AVT_HIP(hipMemcpyAsync(status, pe->d_status, n * sizeof(unsigned), hipMemcpyDeviceToHost, pe->stream));
    AVT_HIP(hipStreamSynchronize(pe->stream));
    if (n_out) *n_out = pe->n_result;
    return 0;
}

}  // namespace

// ---- exported entry points: no C++ exception crosses the C ABI
extern "C" {

int avt_poseerr_create(int device, int V, int J, int num_parts, const int* vertex_part, int max_pairs, avt_poseerr** out) {
    return avt_guard("avt_poseerr_create", [&]() -> int { return create_impl(device, V, J, num_parts, vertex_part, max_pairs, out); });
}

int avt_poseerr_create_for_model(int device, const struct avt_model* model, int num_parts, const int* part_map, int max_pairs, avt_poseerr** out) {
    return avt_guard("avt_poseerr_create_for_model", [&]() -> int { return create_for_model_impl(device, model, num_parts, part_map, max_pairs, out); });
}

void avt_poseerr_destroy(avt_poseerr* pe) {
    if (!pe) return;
    // the buffers go with `delete`, after the stream: it is drained first, so nothing is queued on them either way
    if (pe->stream) (void)hipStreamSynchronize(pe->stream);
    if (pe->ev_in) (void)hipEventDestroy(pe->ev_in);
    if (pe->ev_out) (void)hipEventDestroy(pe->ev_out);
    if (pe->stream) (void)hipStreamDestroy(pe->stream);
    delete pe;
}

int avt_poseerr_upload(avt_poseerr* pe, int side, int n, const double* clouds, const double* joints) {
    return avt_guard("avt_poseerr_upload", [&]() -> int { return upload_impl(pe, side, n, clouds, joints); });
}

int avt_poseerr_from_ctx(avt_poseerr* pe, int side, struct avt_ctx* ctx, int n, const int* frames) {
    return avt_guard("avt_poseerr_from_ctx", [&]() -> int { return from_ctx_impl(pe, side, ctx, n, frames); });
}

int avt_poseerr_run(avt_poseerr* pe) {
    return avt_guard("avt_poseerr_run", [&]() -> int { return run_impl(pe); });
}

int avt_poseerr_get(avt_poseerr* pe, double* summary, double* per_joint, double* per_part, int* argmax, unsigned int* status, int* n) {
    return avt_guard("avt_poseerr_get", [&]() -> int { return get_impl(pe, summary, per_joint, per_part, argmax, status, n); });
}

int avt_poseerr_part_sizes(avt_poseerr* pe, int* sizes, int* V, int* J, int* num_parts) {
    if (!pe) { avt_set_error("avt_poseerr_part_sizes: null scorer"); return 1; }
    if (sizes) std::copy(pe->part_size.begin(), pe->part_size.end(), sizes);
    if (V) *V = pe->V;
    if (J) *J = pe->J;
    if (num_parts) *num_parts = pe->P;
    return 0;
}

int avt_poseerr_sync(avt_poseerr* pe) {
    if (!pe) { avt_set_error("avt_poseerr_sync: null scorer"); return 1; }
    if (pe->device < 0) { avt_set_error(kHostOnly); return 1; }
    AVT_HIP(hipStreamSynchronize(pe->stream));
    return 0;
}

}  // extern "C"
