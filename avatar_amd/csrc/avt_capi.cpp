// avt_capi.cpp — the C ABI of include/avt.h: context management, host<->device staging and the launch
// sequence of AvatarOptimizer::optimize() (AvatarOptimizer.cpp:1246-1517).  Compiled with hipcc (host only).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>

#include <memory>
#include <mutex>

#include "avt_internal.h"

static std::mutex g_graph_mutex;      // every hipGraph call of the process (see run_optimize)

int avt_solve_set_attributes();
int avt_eval_set_attributes();
int avt_render_enqueue(avt_ctx* c, int nframes, const int* d_vertex_part, unsigned long long* d_zkey, unsigned char* d_label, int* d_block,
                       double fx, double fy, double cx, double cy, int width, int height);
int avt_paint_enqueue(avt_ctx* c, int nframes, const int* d_vertex_part, unsigned long long* d_dkey, unsigned long long* d_mkey, float* d_fkey,
                      int* d_frank, unsigned char* d_fedge, float* d_depth, unsigned char* d_label, int* d_block, double fx, double fy, double cx,
                      double cy, int width, int height);
void avt_eval_report_occupancy(const AvtDims& d);

namespace {

template <class T>
int dev_alloc(avt_ctx* c, T** p, size_t n) {
    DevBuf<char> b;
    if (b.reserve(std::max<size_t>(n, 1) * sizeof(T))) return 1;   // an empty table still gets a pointer the kernels may be handed
    *p = (T*)b.p;
    c->owned.push_back(std::move(b));
    return 0;
}
template <class T>
int dev_upload(avt_ctx* c, T** p, const std::vector<T>& v) {
    if (dev_alloc(c, p, v.size())) return 1;
    // (never the legacy stream: another thread of the host may be capturing a graph, and the legacy stream synchronises with it)
    if (!v.empty()) {
        AVT_HIP(hipMemcpyAsync(*p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, c->stream));
        AVT_HIP(hipStreamSynchronize(c->stream));
    }
    return 0;
}

// frame groups of one optimize(): measured on MI355X, two groups pay off from ~32 frames, more never do (avt_tuning::groups overrides)
int choose_groups(int nframes, const avt_tuning& tun) {
    // two groups from 44 frames on - measured, round 5 (moment form from 8 frames per launch on), ms per step one / two groups: 16 frames 0.737 / 0.798, 24: 0.777 / 0.822,
    // 32: 0.810 / 0.838, 36: 0.865 / 0.878, 40: 0.880 / 0.892, 44: 0.938 / 0.913, 48: 0.952 / 0.928, 64: 1.077 / 1.011 (round 4, rows below 64 frames: the crossover was 32)
    int n = nframes >= 44 ? 2 : 1;
    if (tun.groups > 0) n = tun.groups;
    return std::max(1, std::min(std::min(n, AVT_MAX_GROUPS), nframes));
}

// Frame groups of one optimize() call.  Two or three frames: one frame per group when the one-frame launch shape has the speculative
// solver workgroups - in a shared launch a rejection saves its factorisation only if every frame of the launch
// rejects, on a stream of its own every frame keeps its own pace (2 frames 0.477 -> 0.457 ms, 3 frames 0.607 -> 0.526; four: 0.637 -> 0.709).
int choose_G(int nframes, int ngroups, const avt_tuning& tun);
int plan_groups(avt_ctx* c, int nf) {
    int ngroups = choose_groups(nf, c->tun);
    if ((nf == 2 || nf == 3) && c->tun.groups <= 0) {
        const int g_keep = c->fb.G;
        c->fb.G = choose_G(1, 1, c->tun);
        if (avt_solve_rides(c, 1)) ngroups = nf;
        c->fb.G = g_keep;
    }
    return ngroups;
}

int choose_G(int nframes, int ngroups, const avt_tuning& tun) {
    // k_eval workgroups per frame.  Up to 64 frames per launch: 768 workgroups = one resident round at 3 per CU (more rounds
    // cost more in partial tiles and prologues than they balance: 128 frames per group 645 k against 609 k GN it/s with twice as
    // many).  From 128 frames per launch on: 1536, two rounds, so that the hardware's dispatch evens out frames with different
    // numbers of matched points (512 frames: 747 k -> 774 k GN it/s; three rounds: 770 k).
    // Two frame groups side by side (from 32 frames on): the evaluation of one group shares the chip with the other group's
    // solves and reductions, and FEWER, longer-lived workgroups per frame win (round 3, tools/g_sweep.sh, ms per step at
    // 512 / 640 / 768 workgroups per launch: 32 frames 0.934 / 0.928 / 0.966; 48: 1.073 / 1.091 / 1.120; 64: 1.227 / 1.246 / 1.271;
    // 96: 1.625 / 1.623 / 1.622; 128: 2.080 / 1.954 / 1.982; 256 frames: 3.73 / 3.64 / 3.50, 1536: 3.50).
    const int target = nframes >= 128 ? 1536 : (ngroups >= 2 ? (nframes <= 40 ? 512 : 640) : 768);
    const int gcap = std::max(2, std::min(AVT_G_MAX, tun.gcap));
    int g = std::max(2, std::min(gcap, target / std::max(1, nframes)));
    // G >= 64 also selects the few-frames launch shapes (strided batches, k_reduce_strip, the trial point set up in k_lbs's
    // grid): they win up to 6 frames (8 frames: 0.762 ms against 0.712 with G = 63; 12: 0.822 / 0.770)
    if (nframes >= 7) g = std::min(g, 63);
    if (tun.g > 0) return std::max(1, std::min(g, tun.g));   // tuning knob, never above the allocation
    return g;
}

// the defaults of avt_tuning, then - ONCE, here - what the environment says (AVT_<FIELD>); unknown AVT_* names are reported
extern "C" char** environ;
avt_tuning tuning_from_environment() {
    avt_tuning t;
    std::memset(&t, 0, sizeof t);
    t.use_graph = 1; t.groups = 0; t.g = 0; t.gcap = 128; t.vis_frame_min = 32; t.ride = 1; t.ride_strips = 0; t.ride_sizing_groups = 0;
    t.asm_parts = 1; t.spec_cost = 1; t.xcd_frames = 1; t.literal_dims = 1; t.nspec = AVT_MAX_SPEC; t.nn_force_part = 0; t.nn_force_vis = 0; t.nn_slab = 1; t.mom_min_frames = 8; t.debug = 0; t.ride_timeout_us = 2000000;
    struct Knob { const char* name; int* field; };
    const Knob knobs[] = {{"AVT_USE_GRAPH", &t.use_graph}, {"AVT_GROUPS", &t.groups}, {"AVT_G", &t.g}, {"AVT_GCAP", &t.gcap}, {"AVT_VIS_FRAME_MIN", &t.vis_frame_min},
                          {"AVT_RIDE", &t.ride}, {"AVT_RIDE_STRIPS", &t.ride_strips}, {"AVT_RIDE_SIZING_GROUPS", &t.ride_sizing_groups}, {"AVT_NSPEC", &t.nspec},
                          {"AVT_NN_FORCE_PART", &t.nn_force_part}, {"AVT_NN_FORCE_VIS", &t.nn_force_vis}, {"AVT_NN_SLAB", &t.nn_slab}, {"AVT_MOM_MIN_FRAMES", &t.mom_min_frames}, {"AVT_ASM_PARTS", &t.asm_parts}, {"AVT_LBS_FRAMES", &t.lbs_frames}, {"AVT_SPEC_COST", &t.spec_cost}, {"AVT_XCD_FRAMES", &t.xcd_frames}, {"AVT_LITERAL_DIMS", &t.literal_dims}, {"AVT_DEBUG", &t.debug}};
    // names other parts of the repository own (the batch split, the Python loader, bench.py, instrumented builds)
    const char* others[] = {"AVT_LIB", "AVT_RCCL_LIB", "AVT_SHARD_LOOPBACK_TIMEOUT_S", "AVT_BENCH_SHARE_GPU0", "AVT_TIMING"};
    for (char** e = environ; e && *e; ++e) {
        if (std::strncmp(*e, "AVT_", 4) != 0) continue;
        const char* eq = std::strchr(*e, '=');
        if (!eq) continue;
        const std::string name(*e, eq - *e);
        const char* val = eq + 1;
        bool known = false;
        for (const Knob& k : knobs) if (name == k.name) { *k.field = atoi(val); known = true; }
        if (name == "AVT_RIDE_TIMEOUT_US") { t.ride_timeout_us = std::max(0ll, atoll(val)); known = true; }
        // the spellings of earlier rounds
        if (name == "AVT_NO_GRAPH") { t.use_graph = 0; known = true; }
        if (name == "AVT_ONE_GROUP") { t.groups = 1; known = true; }
        if (name == "AVT_NO_RIDE") { t.ride = 0; known = true; }
        if (name == "AVT_NN_NO_SLAB") { t.nn_slab = 0; known = true; }
        if (name == "AVT_RIDE_SIZING") { t.ride_sizing_groups = std::strcmp(val, "groups") == 0; known = true; }
        for (const char* o : others) if (name == o) known = true;
        if (!known) fprintf(stderr, "libavatar_hip: environment variable %s is not a knob of this library (include/avt.h, avt_tuning) - ignored\n", name.c_str());
    }
    return t;
}

int validate_tuning(const avt_tuning& t) {
    if (t.groups < 0 || t.groups > AVT_MAX_GROUPS || t.g < 0 || t.gcap < 2 || t.vis_frame_min < 0 || t.nspec < 0 || t.nspec > AVT_MAX_SPEC ||
        (t.ride_strips != 0 && t.ride_strips != 4 && t.ride_strips != 8) || t.mom_min_frames < 1 || t.ride_timeout_us < 0 || (t.lbs_frames != 0 && t.lbs_frames != 1 && t.lbs_frames != 2 && t.lbs_frames != 4) || t.spec_cost < 0 || t.spec_cost > 1 || t.xcd_frames < 0 || t.xcd_frames > 1 || t.literal_dims < 0 || t.literal_dims > 1 || t.nn_force_vis < 0 || t.nn_force_vis > 1) {
        avt_set_error("avt_tuning: a field is out of range (include/avt.h)");
        return 1;
    }
    return 0;
}

hipEvent_t next_event(avt_ctx* c) {
    if (c->event_pool_used == c->event_pool.size()) {
        hipEvent_t e;
        (void)hipEventCreate(&e);
        c->event_pool.push_back(e);
    }
    return c->event_pool[c->event_pool_used++];
}

struct ProfScope {
    avt_ctx* c;
    int cls;
    hipEvent_t a, b;
    bool on;
    ProfScope(avt_ctx* c_, int cls_) : c(c_), cls(cls_) {
        on = c->profiling && ((c->prof_mask >> cls_) & 1u);
        if (on) { a = next_event(c); b = next_event(c); (void)hipEventRecord(a, c->stream); }
    }
    ~ProfScope() {
        if (on) { (void)hipEventRecord(b, c->stream); c->prof_events.push_back({cls, {a, b}}); }
    }
};

int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { avt_set_error(std::string(what) + ": " + hipGetErrorString(e)); return 1; }
    return 0;
}

// One read-back: the device is selected, the copies are queued on the context's stream behind everything that is queued there
// already, and the host waits once.  A copy whose destination is null - an output the caller did not ask for - is left out.
struct ReadBack { void* dst; const void* src; size_t bytes; };
int read_back(avt_ctx* c, std::initializer_list<ReadBack> copies) {
    AVT_HIP(hipSetDevice(c->device));
    for (const ReadBack& r : copies)
        if (r.dst) AVT_HIP(hipMemcpyAsync(r.dst, r.src, r.bytes, hipMemcpyDeviceToHost, c->stream));
    AVT_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

// What the last search left for `frame` - the counts and sums, the gated and the trimmed matches - is there after a stand-alone
// avt_nn (frame slot 0) and after an optimize call with an ICP iteration on the resident frames: its closing launch resets no
// bookkeeping (LbsLaunch::vis_init = -1).  `who`: the entry point, for the message.
int last_search_left(const avt_ctx* c, const char* who, int frame) {
    const bool after_nn = c->nn_sums_frame0 && !c->frames_valid && frame == 0;
    const bool after_opt = c->frames_valid && c->ran_icp_iters > 0 && frame < c->nframes;
    if (!after_nn && !after_opt) { avt_set_error(std::string(who) + ": neither a stand-alone avt_nn (frame 0) nor an optimize call with an ICP iteration has run last"); return 1; }
    return 0;
}

// Settings the kernels read from device memory - the option scalars, the gate, the trim set, the budgets - are not kernel argument
// values, so that a change replays the same captured graphs; they are on the context's stream, behind every search already queued.
// `held` is the host's record of what the device block holds: when the first n values of it are `want` nothing happens, else `held`
// becomes `want` and `send(held.data())` enqueues it (a failed send leaves no record).  wait: `send` is an asynchronous copy, which
// reads `held` when the stream gets to it - the host waits in front of rewriting `held`, for a copy that an earlier, failed call may
// have left queued on it, and behind the copy, which must have read `held` before the next call rewrites it.  Without: `send`
// launches kernels that carry the values as arguments, read at the launch.
template <class T, class Send>
int upload_when_changed(avt_ctx* c, std::vector<T>& held, const T* want, size_t n, bool wait, Send send) {
    if (held.size() >= n && std::memcmp(want, held.data(), n * sizeof(T)) == 0) return 0;
    AVT_HIP(hipSetDevice(c->device));
    if (wait) AVT_HIP(hipStreamSynchronize(c->stream));
    held.assign(want, want + n);
    if (send(held.data())) { held.clear(); return 1; }
    if (wait) AVT_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

// A per-part setting arrives as n = 0 (off), 1 (every part alike) or num_parts values.  refusal(i): why value i is refused, empty
// when it is not; refusal(-1), asked first: the same for what the setter takes beside the values.
template <class Refusal>
int check_per_part(const char* who, int n, int np, Refusal refusal) {
    if (n != 0 && n != 1 && n != np) {
        avt_set_error(std::string(who) + ": " + std::to_string(n) + " values; 0 (off), 1 (every part) or num_parts = " + std::to_string(np) + " wanted");
        return 1;
    }
    for (int i = -1; i < n; ++i) {
        const std::string why = refusal(i);
        if (!why.empty()) { avt_set_error(std::string(who) + ": " + why); return 1; }
    }
    return 0;
}
// ... and as num_parts values: `off` where n is 0
std::vector<double> per_part(int n, int np, const double* v, double off) {
    std::vector<double> out((size_t)np, off);
    for (int q = 0; q < np && n > 0; ++q) out[(size_t)q] = v[n == 1 ? 0 : q];
    return out;
}

// the launch sequence of one optimize() over the resident frames.  budget (avt_optimize_resident_budgets; nullptr for every other call):
// the per-frame ICP budgets in device memory - the frames whose budget ends early are held where it ends and put back at the end
void enqueue_optimize(avt_ctx* c, const avt_options* o, int f0, int nf, hipStream_t stream, const int* budget = nullptr) {
    c->fb.f0 = f0;
    c->fb.max_iters = o->max_iters_per_icp;
    c->cur_stream = stream;
    c->ran_icp_iters = 0;
    const int vis_init = o->enable_occlusion ? 0 : 1, gn_iters = o->max_iters_per_icp;
    c->lbs_cleared = true;
    // The two passes of the data bucketing ride in the trailing workgroups of the two launches they do not depend on (the label
    // histogram beside the skinning, the scatter beside the visibility pass of the first ICP iteration): two launches fewer on
    // the dependency chain; k_finalize restores the cursors.  (No ICP iteration: the stand-alone launches, cursors cleared.)
    const bool fuse_bucket = o->icp_iters > 0;
    // Few frames (the latency shape, G >= 64): the trial point of every ICP iteration (trial := current + its skeleton tables)
    // is set up by a workgroup in the grid of the k_lbs launch in front of it instead of by a k_solve INIT launch behind k_records.
    // (round 6: small frame batches on the moment form too - up to 16 frames per launch: 0.737 -> 0.726 ms; the launch then asks for the
    // workgroup's 90 KB of LDS for EVERY workgroup of the skinning, one per CU, and at 32 frames per launch that costs more than the INIT launch
    // saves: 0.980 -> 0.990 ms.  The row form's batches need k_solve INIT's deal of the evaluation ranges.)
    const bool fuse_init = (c->fb.G >= 64 || (c->fb.use_moments && nf <= 16)) && avt_lbs_can_init(c->dm.d);
    // budget b: held behind the closing launch of ICP iteration b - 1 (budget 0: the state the call found and its skinning, in two
    // parts); behind the call's closing launch, the held frames are put back
    const bool hold = budget && o->icp_iters > 0;
    if (hold) launch_budget_hold(c, nf, budget, c->budget_hold, 0, false, 1);
    if (!fuse_bucket) { ProfScope ps(c, AVT_K_BUCKET); launch_bucket(c, nf, true); }
    // frame batches: k_compact gathers its candidates from the cloud, so k_lbs does not write the part-sorted copy of it
    const bool few = avt_nn_few(c, nf);
    c->nn_from_cloud = !few;
    const bool mom = c->fb.use_moments != 0, rides = !mom && avt_solve_rides(c, nf);      // rides - few frames, row form: the reduction is part of the solve's launch
    {   // ava.update() precondition (:1356)
        LbsLaunch first;
        first.from_state = 1; first.vis_init = vis_init; first.with_bucket_count = fuse_bucket; first.with_init = fuse_init && o->icp_iters > 0; first.write_pc = few;
        ProfScope ps(c, AVT_K_LBS);
        launch_lbs(c, nf, first);
    }
    if (hold) launch_budget_hold(c, nf, budget, c->budget_hold, 0, false, 2);
    // the normal equations of the trial point.  Moment form (avt_moments.hip): assembled from the correspondences' sufficient statistics -
    // no Jacobian rows, no partial tiles, no reduction.  Row form: k_eval, and k_reduce where the reduction does not ride.
    auto evaluate = [&](int next_seq) {
        if (mom) { ProfScope ps(c, AVT_K_EVAL); launch_assemble(c, nf); return; }
        { ProfScope ps(c, AVT_K_EVAL); launch_eval(c, nf, false, next_seq); }
        if (!rides) { ProfScope ps(c, AVT_K_REDUCE); launch_reduce(c, nf); }
    };
    for (int icp = 0; icp < o->icp_iters; ++icp) {
        { ProfScope ps(c, AVT_K_VISIBILITY); launch_visibility(c, nf, o->enable_occlusion, fuse_bucket && icp == 0); }
        { ProfScope ps(c, AVT_K_NN); launch_nn(c, nf); if (c->trim_on) launch_trim(c, nf); }
        { ProfScope ps(c, AVT_K_AGGREGATE); launch_finalize(c, nf); if (!mom) launch_records(c, nf); }
        if (mom) { ProfScope ps(c, AVT_K_MOMENTS); c->fb.const_used = (c->launch_maxN + 2047) / 2048; launch_moments(c, nf); }      // once per ICP iteration
        if (!fuse_init) { ProfScope ps(c, AVT_K_PREPARE); launch_solve(c, nf, SOLVE_INIT); }
        evaluate(1);
        for (int it = 1; it <= std::max(1, gn_iters); ++it) {
            { ProfScope ps(c, AVT_K_SOLVE); launch_solve(c, nf, it == 1 ? SOLVE_FIRST : SOLVE_NORMAL, it); }
            if (gn_iters == 0) break;
            if (mom || it < gn_iters) evaluate(it + 1);
            else { ProfScope ps(c, AVT_K_DECIDE); launch_eval(c, nf, true); }      // no solve follows the last trial point: its cost alone; the accept test is taken by the closing k_lbs launch
        }
        // moment form, the accept test of the last trial point: the decision part of the solve kernel alone (SOLVE_DECIDE: no factorisation, no step)
        if (mom && gn_iters > 0) { ProfScope ps(c, AVT_K_DECIDE); launch_solve(c, nf, SOLVE_DECIDE, gn_iters + 1); }
        {   // the closing update() of the ICP iteration (:1494-1497), from the skeleton tables of the current point.  The last one of the
            // call skins only - no bookkeeping reset, no trial point, no part-sorted copy - and writes the result records.
            const bool more = icp + 1 < o->icp_iters;
            LbsLaunch close;
            close.from_state = 2; close.vis_init = more ? vis_init : -1; close.with_init = fuse_init && more; close.write_pc = few && more; close.pack = !more;
            close.decide = !mom && gn_iters > 0;      // (the moment form has taken the accept test already)
            ProfScope ps(c, AVT_K_LBS);
            launch_lbs(c, nf, close);
        }
        c->ran_icp_iters++;
        if (hold) launch_budget_hold(c, nf, budget, c->budget_hold, c->ran_icp_iters, c->ran_icp_iters == o->icp_iters);
    }
    c->lbs_cleared = false;
    c->nn_from_cloud = false;
    c->fb.f0 = 0;
    c->cur_stream = c->stream;
}

// the option scalars the kernels read live in device memory (AvtRunParams): uploaded only when they change
int sync_params(avt_ctx* c, const avt_options* o) {
    AvtRunParams pr;
    std::memset(&pr, 0, sizeof pr);
    pr.beta_pose = o->beta_pose; pr.beta_shape = o->beta_shape; pr.lambda0 = o->lm_lambda0;
    pr.lm_up = o->lm_up; pr.lm_down = o->lm_down; pr.lm_min = o->lm_lambda_min; pr.lm_max = o->lm_lambda_max; pr.lm_policy = o->lm_policy == 1 ? 1.0 : 0.0;
    pr.ftol = o->function_tolerance;
    return upload_when_changed(c, c->params_host, &pr, 1, true, [&](const AvtRunParams* src) -> int {
        AVT_HIP(hipMemcpyAsync((void*)c->fb.params, src, sizeof pr, hipMemcpyHostToDevice, c->stream));
        return 0;
    });
}

constexpr size_t GRAPH_CACHE_ENTRIES = 8;

// which form of the data term an optimize() over nf resident frames runs (include/avt.h, avt_set_data_term): ONE rule for run_optimize,
// avt_launch_shape and avt_get_normal_equations.  AUTO: the moment form from tun.mom_min_frames frames per launch on.
bool choose_moments(const avt_ctx* c, int nf) {
    const int g0 = choose_groups(nf, c->tun), per_launch = (nf + g0 - 1) / g0;
    return c->dm.d.mom_ok && (c->data_term == AVT_DATA_TERM_MOMENTS || (c->data_term == AVT_DATA_TERM_AUTO && per_launch >= c->tun.mom_min_frames));
}

// what exists for the resident correspondences after an optimize() call has been enqueued - by launches, by a fresh capture or by the
// replay of a cached graph alike (set inside enqueue_optimize these flags described the last CAPTURED graph, not the last one run)
void note_products(avt_ctx* c, const avt_options* o) {
    if (o->icp_iters > 0) { c->have_moments = c->fb.use_moments != 0; c->have_records = !c->have_moments; }
    c->results_fresh = o->icp_iters > 0;      // the closing k_lbs launch of the call wrote fb.results (no ICP iteration: no closing launch)
}

// what run_optimize checks before anything changes on the device
int check_optimize(const avt_ctx* c, const avt_options* o) {
    const int nf = c->nframes;
    if (nf <= 0 || !c->frames_valid) { avt_set_error("avt_optimize: no frames resident (upload frames first; the stand-alone entry points avt_nn / avt_visibility / avt_lbs_update invalidate them)"); return 1; }
    if (!c->state_valid) { avt_set_error("avt_optimize: no start state resident for these frames (avt_state_upload)"); return 1; }
    if (o->max_iters_per_icp < 0 || o->max_iters_per_icp > 62 || o->icp_iters < 0) { avt_set_error("avt_optimize: bad iteration counts"); return 1; }
    if (o->lm_policy != 0 && o->lm_policy != 1) { avt_set_error("avt_optimize: lm_policy must be 0 (fixed factors) or 1 (gain ratio)"); return 1; }
    if (!(o->lm_up > 1.0) || !(o->lm_down > 0.0 && o->lm_down < 1.0)) { avt_set_error("avt_optimize: lm_up must be > 1 and lm_down in (0, 1)"); return 1; }
    if (!(o->function_tolerance >= 0.0 && o->function_tolerance < 1.0)) { avt_set_error("avt_optimize: function_tolerance must be in [0, 1) (0 = no early exit)"); return 1; }
    return 0;
}

// ---- the graph cache: the launch sequence depends only on the launch shape, so it is captured once per shape and replayed afterwards.
// Every graph call of the process goes through g_graph_mutex: contexts are per thread, but HIP 7.0's hipGraphLaunch is not safe
// against a hipGraphLaunch from another thread (found by the 8-thread loop-back tests: SIGSEGV in hip::Graph::UpdateStreams <-
// hip::GraphExec::Run, which rearranges a per-device set of helper streams for graphs with parallel branches).  The calls only
// enqueue, so the lock is held for microseconds.  graph_drop_all takes it; the other two are called with it held (run_optimize).

// every launch sequence captured so far goes: what it was made with - knobs, scratch, the context itself - is about to change
void graph_drop_all(avt_ctx* c) {
    std::lock_guard<std::mutex> graph_lock(g_graph_mutex);
    for (auto& e : c->graphs) (void)hipGraphExecDestroy(e.exec);
    c->graphs.clear();
}

// room for one more: the least recently used launch shape goes, once nothing queued replays it any more
int graph_evict(avt_ctx* c) {
    if (c->graphs.size() < GRAPH_CACHE_ENTRIES) return 0;
    size_t lru = 0;
    for (size_t i = 1; i < c->graphs.size(); ++i) if (c->graphs[i].last_used < c->graphs[lru].last_used) lru = i;
    AVT_HIP(hipStreamSynchronize(c->stream));
    (void)hipGraphExecDestroy(c->graphs[lru].exec);
    c->graphs.erase(c->graphs.begin() + lru);
    return 0;
}

// the cached graph of this call's launch shape; captured - the frame groups as parallel branches - when the shape is new
int graph_find_or_capture(avt_ctx* c, const avt_options* o, int ngroups, int nfg, const int* budget, avt_ctx::GraphEntry** out) {
    const int nf = c->nframes;
    char key[200];
    snprintf(key, sizeof key, "%d|%d|%d|%d|%d|%d|%d|%d|%dx%d%s%s", nf, ngroups, c->fb.G, c->launch_maxN, o->icp_iters, o->max_iters_per_icp, o->enable_occlusion, c->fb.use_moments,
             c->occ_w, c->occ_w > 0 ? c->occ_h : 0, budget ? "|budgets" : "",      // (the budgets themselves live in device memory: a changing pattern replays the same graph)
             c->trim_on ? "|trim" : "");                                            // (one launch more per search; its settings live in device memory too)
    for (auto& e : c->graphs) if (e.key == key) { *out = &e; return 0; }
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    AVT_HIP(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    bool bad = false;
    auto cap = [&](hipError_t e) { if (e != hipSuccess && !bad) { bad = true; avt_set_error(std::string("optimize graph capture: ") + hipGetErrorString(e)); } };
    if (ngroups > 1) cap(hipEventRecord(c->ev_fork, c->stream));
    for (int gi = 1; gi < ngroups; ++gi) cap(hipStreamWaitEvent(c->side[gi - 1], c->ev_fork, 0));
    for (int gi = 0; gi < ngroups; ++gi) {
        const int f0 = gi * nfg, n = std::min(nfg, nf - f0);
        if (n > 0) enqueue_optimize(c, o, f0, n, gi == 0 ? c->stream : c->side[gi - 1], budget);
    }
    for (int gi = 1; gi < ngroups; ++gi) {
        cap(hipEventRecord(c->ev_join[gi - 1], c->side[gi - 1]));
        cap(hipStreamWaitEvent(c->stream, c->ev_join[gi - 1], 0));
    }
    cap(hipGetLastError());
    // the capture is ALWAYS ended, so that a failure does not leave the stream stuck in capture mode
    const hipError_t ee = hipStreamEndCapture(c->stream, &graph);
    if (bad || ee != hipSuccess) {
        if (!bad) avt_set_error(std::string("hipStreamEndCapture: ") + hipGetErrorString(ee));
        if (graph) (void)hipGraphDestroy(graph);
        return 1;
    }
    const hipError_t ei = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ei != hipSuccess) { avt_set_error(std::string("hipGraphInstantiate: ") + hipGetErrorString(ei)); return 1; }
    if (graph_evict(c)) return 1;
    c->graphs.push_back({key, exec, 0});
    *out = &c->graphs.back();
    return 0;
}

// One optimize() over the resident frames: choose the launch shape, run it - launch by launch, or as the replay of its graph - and
// note what it leaves.  budget: see enqueue_optimize (nullptr: a plain call, whose launch sequence and graphs do not know about budgets)
int run_optimize(avt_ctx* c, const avt_options* o, const int* budget = nullptr) {
    const int nf = c->nframes;
    if (check_optimize(c, o)) return 1;
    if (sync_params(c, o)) return 1;
    c->ran_max_iters = o->max_iters_per_icp;
    if (o->icp_iters > 0) c->trim_last = c->trim_on;      // (no ICP iteration: no search, the last one's counts stand)
    // The shape.  Large batches run as several frame groups: the latency-bound single-workgroup-per-frame kernels of one group
    // (k_solve, k_finalize, k_reduce) overlap the throughput kernels (k_eval, k_nn) of the others on separate streams.
    c->fb.use_moments = choose_moments(c, nf);      // which form of the data term this call runs
    c->last_run_moments = c->fb.use_moments != 0;
    const int ngroups = plan_groups(c, nf);
    const int nfg = (nf + ngroups - 1) / ngroups;       // frames per group (the last group may be smaller)
    c->fb.G = choose_G(nfg, ngroups, c->tun);
    c->concurrent_groups = ngroups;
    int rc = 0;
    if (!c->tun.use_graph || c->profiling) {
        // The instrumented (profiling) path keeps the SAME groups and launch shapes and runs them one after the other on
        // the main stream, so that per-launch timings describe the launches the graph replays.
        for (int gi = 0; gi < ngroups; ++gi) {
            const int f0 = gi * nfg, n = std::min(nfg, nf - f0);
            if (n > 0) enqueue_optimize(c, o, f0, n, c->stream, budget);
        }
        rc = check_launch("optimize launch sequence");
    } else {
        std::lock_guard<std::mutex> graph_lock(g_graph_mutex);
        avt_ctx::GraphEntry* hit = nullptr;
        if (graph_find_or_capture(c, o, ngroups, nfg, budget, &hit)) return 1;
        hit->last_used = ++c->graph_clock;
        AVT_HIP(hipGraphLaunch(hit->exec, c->stream));
    }
    c->ran_icp_iters = o->icp_iters;
    note_products(c, o);
    return rc;
}

// The context's record of which frames are resident: `count_of(f)` points in frame f.  The counts are validated first - nothing changes when it
// fails - then nframes, frame_N, frame_off and launch_maxN are written, and what described the old frames' correspondences and results is dropped.
// frames_valid / state_valid are the caller's.  (A callable, not an array: the host-to-host call has offsets and must not allocate.)
template <class CountOf>
int set_resident_frames(avt_ctx* c, int nframes, CountOf count_of) {
    if (nframes <= 0 || nframes > c->fb.max_frames) { avt_set_error("frames: nframes out of range for this context"); return 1; }
    int mx = 0;
    for (int f = 0; f < nframes; ++f) {
        const int n = count_of(f);
        if (n < 0) { avt_set_error("frames: negative point count (frame_offsets must be non-decreasing)"); return 1; }
        if (n > c->fb.max_points) { avt_set_error("frames: a frame has more points than max_points_per_frame"); return 1; }
        mx = std::max(mx, n);
    }
    c->sub.pending = false;                         // whatever installs frames takes the slots of a pending subsampled batch
    c->have_moments = c->have_records = false;      // new frames: the moments / records of the old correspondences describe nothing resident
    c->results_fresh = false;
    c->nframes = nframes;
    c->frame_N.resize(nframes);
    c->frame_off.assign(nframes + 1, 0);
    for (int f = 0; f < nframes; ++f) { c->frame_N[f] = count_of(f); c->frame_off[f + 1] = c->frame_off[f] + c->frame_N[f]; }
    c->launch_maxN = std::max(mx, std::min(c->fb.max_points, ((mx + 2047) / 2048) * 2048));
    return 0;
}

// The closing step of an install: the point counts of the resident frames go into the device control blocks (working copy and
// start copy), the host waits, and the frames count as resident.
int publish_frames(avt_ctx* c, int nframes, bool same_shape) {
    for (AvtFrameCtl* dst : {c->fb.ctl, c->fb.ctl_start})
        AVT_HIP(hipMemcpy2DAsync(&dst->N, sizeof(AvtFrameCtl), c->frame_N.data(), sizeof(int), sizeof(int), (size_t)nframes, hipMemcpyHostToDevice, c->stream));
    AVT_HIP(hipStreamSynchronize(c->stream));
    c->frames_valid = true;
    if (!same_shape) c->state_valid = false;     // a different number of frames needs a new start state
    return 0;
}

// ---- staging: what the staged calls (avt_frames_upload, avt_state_upload, avt_state_download below) and the host-pointer calls share

// the points and labels of the resident frames into their slots: data / labels are packed back to back (frame f starts at the sum
// of the previous counts) in host memory or, kind = device to device, in device memory (the batch split's receive buffer)
int enqueue_frame_copies(avt_ctx* c, const double* data, const int* labels, hipMemcpyKind kind) {
    for (int f = 0; f < c->nframes; ++f) {
        const size_t N = (size_t)c->frame_N[f], o = (size_t)c->frame_off[f];
        if (N == 0) continue;
        AVT_HIP(hipMemcpyAsync(c->fb.data_raw + (size_t)f * c->fb.max_points * 3, data + o * 3, N * 3 * sizeof(double), kind, c->stream));
        AVT_HIP(hipMemcpyAsync(c->fb.labels_raw + (size_t)f * c->fb.max_points, labels + o, N * sizeof(int), kind, c->stream));
    }
    return 0;
}

// The start states and control blocks of the resident frames, [x | ctl] as the device holds them, filled into `block` (caller's, of
// state_block_bytes, 8-byte aligned) and sent to the working copy and the start copy.  The caller waits before `block` goes.
size_t state_block_bytes(const avt_ctx* c, int nframes) { return (size_t)nframes * (2 * c->dm.d.xsize * sizeof(double) + sizeof(AvtFrameCtl)); }
int enqueue_start_states(avt_ctx* c, int nframes, void* block, const double* p, const double* q, const double* w) {
    const AvtDims& d = c->dm.d;
    const size_t b_x = (size_t)nframes * 2 * d.xsize * sizeof(double), b_ctl = (size_t)nframes * sizeof(AvtFrameCtl);
    double* xs = (double*)block;
    AvtFrameCtl* ctl = (AvtFrameCtl*)((char*)block + b_x);
    std::memset(block, 0, b_x + b_ctl);
    for (int f = 0; f < nframes; ++f) {
        pack_state_row(d, xs + (size_t)f * 2 * d.xsize, p, q, w, f);
        ctl[f].N = c->frame_N[f];
        ctl[f].comp_cur = -1;
    }
    if (nframes == c->fb.max_frames) {      // [x | ctl] and [x_start | ctl_start] are contiguous on the device as they are in the block
        AVT_HIP(hipMemcpyAsync(c->fb.x, xs, b_x + b_ctl, hipMemcpyHostToDevice, c->stream));
        AVT_HIP(hipMemcpyAsync(c->fb.x_start, xs, b_x + b_ctl, hipMemcpyHostToDevice, c->stream));
    } else {
        AVT_HIP(hipMemcpyAsync(c->fb.x, xs, b_x, hipMemcpyHostToDevice, c->stream));
        AVT_HIP(hipMemcpyAsync(c->fb.ctl, ctl, b_ctl, hipMemcpyHostToDevice, c->stream));
        AVT_HIP(hipMemcpyAsync(c->fb.x_start, c->fb.x, b_x, hipMemcpyDeviceToDevice, c->stream));
        AVT_HIP(hipMemcpyAsync(c->fb.ctl_start, c->fb.ctl, b_ctl, hipMemcpyDeviceToDevice, c->stream));
    }
    return 0;
}

// A faulty frame anywhere: nothing is handed back.  fault_of(f) is frame f's fault word; the first faulty frame is reported, once -
// the words are cleared, the next optimize() starts clean.
template <class FaultOf>
int check_device_faults(avt_ctx* c, int nframes, FaultOf fault_of) {
    int first = -1, nbad = 0;
    unsigned bits = 0;
    for (int f = 0; f < nframes; ++f)
        if (const unsigned b = fault_of(f)) { if (first < 0) { first = f; bits = b; } ++nbad; }
    if (first < 0) return 0;
    char msg[256];
    snprintf(msg, sizeof msg, "optimize: %d frame(s) carry a device fault (first: frame %d, bits 0x%x%s); their result is not valid", nbad, first,
             bits, (bits & AVT_FAULT_RIDE_TIMEOUT) ? ": a solver gave up waiting for the in-launch reduction" : "");
    if (avt_internal_clear_faults(c)) return 1;
    avt_set_error(msg);
    return AVT_STATUS_DEVICE_FAULT;
}

// Installs `nframes` frames with `count_of(f)` points each, from host memory or, with device_src, from device memory.
// Everything is validated before any host or device state changes.  The per-frame point count is also written into the
// device control blocks (working copy and start copy), so that swapping frames under a resident state - the warm-start
// pattern avt_frames_upload + avt_optimize_resident - runs with the new counts.
template <class CountOf>
int install_frames(avt_ctx* c, int nframes, CountOf count_of, const double* data, const int* labels, bool device_src) {
    const bool same_shape = c->frames_valid && nframes == c->nframes;
    if (set_resident_frames(c, nframes, count_of)) return 1;
    c->frames_valid = false;
    if (enqueue_frame_copies(c, data, labels, device_src ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice)) return 1;
    return publish_frames(c, nframes, same_shape);
}

int upload_frames(avt_ctx* c, int nframes, const double* data, const int* labels, const int* offs) {
    const size_t first = nframes > 0 ? (size_t)offs[0] : 0;      // (a bad nframes is install_frames' to reject: no entry of offs is read for it)
    return install_frames(c, nframes, [&](int f) { return offs[f + 1] - offs[f]; }, data + first * 3, labels + first, false);
}

// avt_optimize / avt_optimize_batch on HOST pointers - the reference's call shape, optimize(const CloudType&, const VectorXi&, ..)
// (AvatarOptimizer.h:17-19) - as one pass with ONE host synchronisation: clouds, labels, start states and control blocks are gathered in
// the context's pinned staging block and leave as asynchronous copies (no pageable-memory staging inside the runtime, no wait between
// them), the fit is enqueued behind them, its closing k_lbs launch (k_pack_results where there is none) puts (p, q, w), the statistics and the fault word of every frame into one block
// and ONE copy brings it back.  (The four-stage path - upload, upload, run, download, a synchronisation each - measured 81 + 26 + 58 us
// on top of the 0.41 ms fit of one 38 k-point frame, tools/host_call_breakdown.py.)  Leaves the context exactly as the staged calls do:
// frames and start state resident, avt_state_reset / avt_optimize_resident usable afterwards.
// (posed_*: optional - frame 0's ava.cloud / jointPos / jointTrans of the closing update(), brought back by the same synchronisation: avt_optimize_posed)
int optimize_host_to_host(avt_ctx* c, int nframes, const double* data, const int* labels, const int* offs, const avt_options* o,
                          double* p, double* q, double* w, avt_stats* st, double* posed_cloud = nullptr, double* posed_jpos = nullptr, double* posed_jtrans = nullptr) {
    const AvtDims& d = c->dm.d;
    if (set_resident_frames(c, nframes, [&](int f) { return offs[f + 1] - offs[f]; })) return 1;
    c->frames_valid = c->state_valid = false;      // until the copies below are enqueued
    const size_t total = (size_t)c->frame_off[nframes];
    const int stride = result_stride(d);
    const size_t b_data = total * 24, b_lab = (total * 4 + 15) & ~(size_t)15, b_state = state_block_bytes(c, nframes), b_res = (size_t)nframes * stride * 8;
    const bool want_posed = posed_cloud || posed_jpos || posed_jtrans;
    const size_t b_cloud = (size_t)3 * d.V * 8, b_jpos = (size_t)3 * d.J * 8, b_jtrans = (size_t)12 * d.J * 8;
    const size_t need = b_data + b_lab + b_state + b_res + (want_posed ? b_cloud + b_jpos + b_jtrans : 0) + 64;
    //  the pinned block grows with the largest call and shrinks again when a call needs less than a quarter of it: a tracker that once
    // fitted a dense 512-frame batch does not keep gigabytes pinned for its one-frame calls
    if (c->host_pin_cap < need || (c->host_pin_cap > (64u << 20) && need < c->host_pin_cap / 4)) {
        AVT_HIP(hipStreamSynchronize(c->stream));
        if (c->host_pin) (void)hipHostFree(c->host_pin);
        c->host_pin = nullptr; c->host_pin_cap = 0;
        const size_t cap = need + need / 4;
        AVT_HIP(hipHostMalloc((void**)&c->host_pin, cap, hipHostMallocDefault));
        c->host_pin_cap = cap;
    }
    // the pinned block: data | labels | x | ctl | result records | posed outputs of frame 0
    char *h_data = c->host_pin, *h_lab = h_data + b_data, *h_state = h_lab + b_lab, *h_res = h_state + b_state, *h_posed = h_res + b_res;
    std::memcpy(h_data, data + (size_t)offs[0] * 3, b_data);
    std::memcpy(h_lab, labels + offs[0], total * 4);
    if (enqueue_frame_copies(c, (const double*)h_data, (const int*)h_lab, hipMemcpyHostToDevice)) return 1;
    if (enqueue_start_states(c, nframes, h_state, p, q, w)) return 1;
    c->frames_valid = c->state_valid = true;
    if (run_optimize(c, o)) { c->results_fresh = false; return 1; }
    if (!c->results_fresh) { launch_pack_results(c, nframes); c->results_fresh = true; }      // (a call without ICP iterations has no closing k_lbs launch)
    // behind the fit, in front of the one synchronisation of the call
    if (read_back(c, {{h_res, c->fb.results, b_res}, {want_posed ? h_posed : nullptr, c->fb.cloud, b_cloud},
                      {want_posed ? h_posed + b_cloud : nullptr, c->fb.jointpos, b_jpos}, {want_posed ? h_posed + b_cloud + b_jpos : nullptr, c->fb.jointtrans, b_jtrans}}))
        return 1;
    const double* res = (const double*)h_res;
    if (const int rc = check_device_faults(c, nframes, [&](int f) { return unpack_result_row(d, res + (size_t)f * stride, nullptr, nullptr, nullptr, nullptr, f); })) return rc;
    if (posed_cloud) std::memcpy(posed_cloud, h_posed, b_cloud);
    if (posed_jpos) std::memcpy(posed_jpos, h_posed + b_cloud, b_jpos);
    if (posed_jtrans) std::memcpy(posed_jtrans, h_posed + b_cloud + b_jpos, b_jtrans);
    for (int f = 0; f < nframes; ++f) unpack_result_row(d, res + (size_t)f * stride, p, q, w, st, f);
    return 0;
}

// The parameters of a stand-alone skinning (Avatar::update of `nframes` avatars) staged in the prep buffer, which nothing else uses
// outside optimize(): w | p | R.  `who`: the entry point, for the message.
// lbs: the k_lbs launch that poses them (the given pose, no bookkeeping touched)
int stage_pose(avt_ctx* c, const char* who, int nframes, const double* w, const double* p, const double* R, LbsLaunch* lbs) {
    const AvtDims& d = c->dm.d;
    if ((size_t)nframes * (d.K + 3 + 9 * d.J) > (size_t)c->fb.max_frames * 2 * d.prep_size) { avt_set_error(std::string(who) + ": staging overflow"); return 1; }
    double *dw = c->fb.prep, *dp = dw + (size_t)nframes * d.K, *dR = dp + (size_t)nframes * 3;
    AVT_HIP(hipMemcpyAsync(dw, w, (size_t)nframes * d.K * sizeof(double), hipMemcpyHostToDevice, c->stream));
    AVT_HIP(hipMemcpyAsync(dp, p, (size_t)nframes * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    AVT_HIP(hipMemcpyAsync(dR, R, (size_t)nframes * 9 * d.J * sizeof(double), hipMemcpyHostToDevice, c->stream));
    lbs->w = dw; lbs->p = dp; lbs->R = dR;
    return 0;
}

}  // namespace

int avt_internal_commit_frames(avt_ctx* c, int nframes, const int* counts, bool same_shape) {
    if (set_resident_frames(c, nframes, [&](int f) { return counts[f]; })) return 1;
    c->frames_valid = false;
    return publish_frames(c, nframes, same_shape);
}

// batch split (avt_shard.cpp): frames received into a device buffer become this context's resident frames
int avt_internal_install_frames(avt_ctx* c, int nframes, const int* counts, const double* data, const int* labels, int device_src) {
    return install_frames(c, nframes, [&](int f) { return counts[f]; }, data, labels, device_src != 0);
}

// a fault is reported once: the next optimize() starts clean, and a later gather packs the result records again
int avt_internal_clear_faults(avt_ctx* c) {
    c->results_fresh = false;      //  the records carry the word that is being cleared
    AVT_HIP(hipMemsetAsync(c->fb.fault, 0, (size_t)c->fb.max_frames * sizeof(unsigned), c->stream));
    AVT_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" {

static int ctx_create_impl(int device, const avt_model* m, int num_parts, const int* part_map, int max_points, int max_frames, avt_ctx** out) {
    if (!m || !part_map || !out) { avt_set_error("avt_ctx_create: null argument"); return 1; }
    if (num_parts <= 0 || num_parts > AVT_MAX_PARTS) { avt_set_error("avt_ctx_create: num_parts out of range (1..64)"); return 1; }
    if (max_points <= 0 || max_frames <= 0) { avt_set_error("avt_ctx_create: max_points/max_frames must be positive"); return 1; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        avt_set_error("avt_ctx_create: no HIP device available (this library has no CPU fallback)");
        return 2;
    }
    if (device < 0 || device >= ndev) { avt_set_error("avt_ctx_create: device index out of range"); return 1; }
    AVT_HIP(hipSetDevice(device));
    avt_ctx* c = new avt_ctx();     // (its member initialisers: every handle starts null, avt_ctx_destroy copes with a partial context)
    *out = c;
    c->device = device;
    c->model = m;
    c->tun = tuning_from_environment();
    if (validate_tuning(c->tun)) return 1;
    { hipDeviceProp_t pr; c->num_cus = hipGetDeviceProperties(&pr, device) == hipSuccess ? pr.multiProcessorCount : 0; }
    AVT_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    AVT_HIP(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    for (int i = 0; i < AVT_MAX_GROUPS - 1; ++i) {
        AVT_HIP(hipStreamCreateWithFlags(&c->side[i], hipStreamNonBlocking));
        AVT_HIP(hipEventCreateWithFlags(&c->ev_join[i], hipEventDisableTiming));
    }
    c->cur_stream = c->stream;
    if (avt_solve_set_attributes() || avt_eval_set_attributes() || avt_lbs_set_attributes() || avt_moments_set_attributes()) { avt_set_error("avt_ctx_create: hipFuncSetAttribute failed"); return 1; }
    DeviceModel& dm = c->dm;
    dm.d = m->d;
    if (!dm.d.mom_ok) c->mom_reason = "K + 1 <= 16 and 3 + 3J + K <= 87 required";
    else if (avt_moments_lds_need(dm.d) > avt_moments_lds_cap()) {      // AUTO then keeps the row form, avt_set_data_term(MOMENTS) says why
        dm.d.mom_ok = 0;
        c->mom_reason = "its assembly needs " + std::to_string(avt_moments_lds_need(dm.d)) + " bytes of LDS per workgroup, " + std::to_string(avt_moments_lds_cap()) + " available";
    }
    // visibility as one workgroup per frame when the frame's x, y fit the LDS
    c->vis_frame_min = avt_visibility_frame_lds(m->d) <= 150 * 1024 ? c->tun.vis_frame_min : 0;
    dm.d.num_parts = num_parts;
    const int V = dm.d.V, J = dm.d.J;
    c->part_map.assign(part_map, part_map + J);   // >= J entries (AvatarOptimizer.cpp:1229)
    // model part buckets (AvatarOptimizer.cpp:1227-1243)
    std::vector<int> pov(V), pstart(num_parts + 1, 0), pverts(V), ppos(V);
    for (int v = 0; v < V; ++v) {
        const int q = part_map[m->main_joint[v]];
        if (q < 0 || q >= num_parts) { avt_set_error("avt_ctx_create: part_map entry out of [0,num_parts)"); return 1; }
        pov[v] = q;
        pstart[q + 1]++;
    }
    for (int q = 0; q < num_parts; ++q) pstart[q + 1] += pstart[q];
    {
        std::vector<int> fill(pstart.begin(), pstart.end() - 1);
        for (int v = 0; v < V; ++v) { const int pos = fill[pov[v]]++; pverts[pos] = v; ppos[v] = pos; }
    }
    if (dev_upload(c, &dm.vrec, m->vrec) || dev_upload(c, &dm.shape_planes, m->shape_planes) || dev_upload(c, &dm.lbs_w, m->lbs_w) || dev_upload(c, &dm.lbs_j, m->lbs_j) ||
        dev_upload(c, &dm.asg_w, m->asg_w) || dev_upload(c, &dm.asg_j, m->asg_j) || dev_upload(c, &dm.anc_n, m->anc_n) ||
        dev_upload(c, &dm.anc, m->anc) || dev_upload(c, &dm.mesh, m->mesh_soa) || dev_upload(c, &dm.parent, m->parent) || dev_upload(c, &dm.jlevel, m->jlevel) || dev_upload(c, &dm.fk_items, m->fk_items) || dev_upload(c, &dm.tile_col, m->tile_col) || dev_upload(c, &dm.deal_col, m->deal_col) || dev_upload(c, &dm.tile_param, m->tile_param) ||
        dev_upload(c, &dm.joint_col, m->joint_col) || dev_upload(c, &dm.vorder, m->vorder) || dev_upload(c, &dm.vmask, m->vmask) || dev_upload(c, &dm.fk_level_off, m->fk_level_off) || dev_upload(c, &dm.fk_titems, m->fk_titems) ||
        dev_upload(c, &dm.jsr_base, m->jsr_base) || dev_upload(c, &dm.jsr, m->jsr) || dev_upload(c, &dm.S, m->S) ||
        dev_upload(c, &dm.Sp, m->Sp) || dev_upload(c, &dm.prior_mean, m->prior_mean) || dev_upload(c, &dm.prior_prec, m->prior_prec) ||
        dev_upload(c, &dm.prior_clog, m->prior_clog) || dev_upload(c, &dm.part_of_vertex, pov) ||
        dev_upload(c, &dm.part_start, pstart) || dev_upload(c, &dm.part_vertices, pverts) || dev_upload(c, &dm.part_pos, ppos) ||
        dev_upload(c, &dm.mom_pair, m->mom_pair) || dev_upload(c, &dm.mom_lstart, m->mom_lstart) || dev_upload(c, &dm.mom_lv, m->mom_lv) || dev_upload(c, &dm.mom_lw, m->mom_lw) ||
        dev_upload(c, &dm.mom_psi, m->mom_psi) || dev_upload(c, &dm.mom_opk_start, m->mom_opk_start) || dev_upload(c, &dm.mom_opk, m->mom_opk) ||
        dev_upload(c, &dm.mom_sub_start, m->mom_sub_start) || dev_upload(c, &dm.mom_sub, m->mom_sub) || dev_upload(c, &dm.mom_m1_start, m->mom_m1_start) ||
        dev_upload(c, &dm.mom_m1, m->mom_m1) || dev_upload(c, &dm.mom_s2_start, m->mom_s2_start) || dev_upload(c, &dm.mom_s2, m->mom_s2) || dev_upload(c, &dm.mom_s2_jj, m->mom_s2_jj) || dev_upload(c, &dm.mom_z2_jj, m->mom_z2_jj) || dev_upload(c, &dm.mom_tab16, m->mom_tab16))
        return 1;
    FrameBuffers& fb = c->fb;
    fb.max_frames = max_frames;
    fb.max_points = max_points;
    fb.G = choose_G(max_frames, 1, c->tun);
    fb.const_blocks = (max_points + 255) / 256;
    fb.bucket_tiles = (max_points + 2047) / 2048;
    const size_t FN = (size_t)max_frames * max_points, FV = (size_t)max_frames * V;
    const AvtDims& d = dm.d;
    // eval workgroups over all frames, for every way run_optimize may split them into groups
    size_t part_cap = 0;
    avt_tuning widest = c->tun;      // (the largest cap a later avt_ctx_set_tuning may ask for)
    widest.gcap = AVT_G_MAX; widest.g = 0;
    for (int nf = 1; nf <= max_frames; ++nf)
        for (int k = 1; k <= std::min(AVT_MAX_GROUPS, nf); ++k) part_cap = std::max(part_cap, (size_t)nf * std::max(choose_G((nf + k - 1) / k, 1, widest), choose_G((nf + k - 1) / k, 2, widest)));
    char* cntsum = nullptr;
    char* state_block = nullptr;
    if (dev_alloc(c, &fb.data_raw, FN * 3) || dev_alloc(c, &fb.labels_raw, FN) || dev_alloc(c, &fb.dx, FN) || dev_alloc(c, &fb.dy, FN) ||
        dev_alloc(c, &fb.dz, FN) || dev_alloc(c, &fb.dorig, FN) || dev_alloc(c, &fb.part_off, (size_t)max_frames * (num_parts + 1)) || dev_alloc(c, &fb.part_cnt, (size_t)max_frames * 2 * (AVT_MAX_PARTS + 1)) || dev_alloc(c, &fb.tile_hist, (size_t)max_frames * ((max_points + 2047) / 2048) * (AVT_MAX_PARTS + 1)) ||
        dev_alloc(c, &fb.corr, FN) || dev_alloc(c, &fb.corr_sorted, FN) || dev_alloc(c, &fb.cloud, FV * 3) || dev_alloc(c, &fb.pcx, FV) ||
        dev_alloc(c, &fb.pcy, FV) || dev_alloc(c, &fb.pcz, FV) || dev_alloc(c, &fb.visible, FV) || dev_alloc(c, &fb.vcx, FV) || dev_alloc(c, &fb.vcy, FV) ||
        dev_alloc(c, &fb.vcz, FV) || dev_alloc(c, &fb.vcid, FV) || dev_alloc(c, &fb.vcount, (size_t)max_frames * num_parts) || dev_alloc(c, &fb.vis_sorted, FV) || dev_alloc(c, &fb.ride_ctr, (size_t)max_frames) || dev_alloc(c, &fb.fault, (size_t)max_frames) || dev_alloc(c, &fb.spec, (size_t)max_frames) || dev_alloc(c, &fb.snap, (size_t)max_frames) || dev_alloc(c, &fb.x_spec, (size_t)max_frames * AVT_MAX_SPEC * d.xsize) || dev_alloc(c, &fb.prep_spec, (size_t)max_frames * AVT_MAX_SPEC * d.prep_size) ||
        dev_alloc(c, &cntsum, FV * (sizeof(int) + 3 * sizeof(long long)) + 64) || dev_alloc(c, &fb.matched, FV) ||
        dev_alloc(c, &fb.const_part, (size_t)max_frames * fb.const_blocks) ||
        dev_alloc(c, &state_block, 2 * ((size_t)max_frames * 2 * d.xsize * sizeof(double) + (size_t)max_frames * sizeof(AvtFrameCtl))) ||
        dev_alloc(c, &fb.prep, (size_t)max_frames * 2 * d.prep_size) ||
        dev_alloc(c, &fb.rec, (size_t)max_frames * d.nb_max * 4 * d.rec_quad) || dev_alloc(c, &fb.partial, part_cap * d.NPAIR * 256) || dev_alloc(c, &fb.wmask, part_cap) || dev_alloc(c, &fb.bmask, (size_t)max_frames * d.nb_max) || dev_alloc(c, &fb.erange, (size_t)max_frames * AVT_ERANGE) || dev_alloc(c, &fb.Hraw, (size_t)max_frames * 2 * d.HS * d.HS) ||
        dev_alloc(c, &fb.prior, (size_t)max_frames * 2 * AVT_MAX_COMPS * AVT_PRIOR_STRIDE) ||
        dev_alloc(c, &fb.jointpos, (size_t)max_frames * 3 * J) || dev_alloc(c, &fb.jointtrans, (size_t)max_frames * 12 * J) ||
        dev_alloc(c, &fb.trace, (size_t)max_frames * 64) || dev_alloc(c, &fb.results, (size_t)max_frames * result_stride(d)))
        return 1;
    {   // the states and control blocks and their start copies are ONE allocation, [x | ctl | x_start | ctl_start]: a context used at its full frame
        // count (the facade's: one frame) uploads state + control block with one copy and keeps the start copy with one more (round 6: they were four)
        const size_t bx = (size_t)max_frames * 2 * d.xsize * sizeof(double), bc = (size_t)max_frames * sizeof(AvtFrameCtl);
        fb.x = (double*)state_block; fb.ctl = (AvtFrameCtl*)(state_block + bx);
        fb.x_start = (double*)(state_block + bx + bc); fb.ctl_start = (AvtFrameCtl*)(state_block + 2 * bx + bc);
    }
    if (d.mom_ok) {      // moment form of the data term (avt_moments.hip): T per (frame, joint pair), D per (frame, joint), scratch of the assembly
        if (dev_alloc(c, &fb.mom_T, (size_t)max_frames * avt_moments_T_doubles(d)) || dev_alloc(c, &fb.mom_D, (size_t)max_frames * J * d.mom_npsi * 3) ||
            dev_alloc(c, &fb.mom_E, (size_t)max_frames * 2) || dev_alloc(c, &fb.mom_rec, (size_t)max_frames * avt_moments_frame_scratch(d)))
            return 1;
        AVT_HIP(hipMemsetAsync(fb.mom_D, 0, (size_t)max_frames * J * d.mom_npsi * 3 * sizeof(double), c->stream));      // joints no vertex is assigned to keep zeros
    }
    // (data_term starts as AUTO; tun.mom_min_frames = 8, round 5 - ms per step moments / rows, frames per launch [frames per GPU]: 4 [4] 0.701 / 0.648, 6 [6] 0.710 / 0.692, 8 [8] 0.709 / 0.724,
    //  12 [12] 0.747 / 0.787, 16 [16] 0.737 / 0.800, 12 [24] 0.777 / 0.877, 16 [32] 0.838 / 0.938, 24 [48] 0.934 / 1.075, 28 [56] 0.985 / 1.186; dense frames 8 [8] 0.757 / 0.777,
    //  16 [16] 0.817 / 0.884; tools/ab_env.sh AVT_MOM_MIN_FRAMES.  Round 4's crossover was 32 frames per launch: the assembly as role workgroups, the decide-only closing
    //  pass and the XCD frame mapping took 15 % off the moment form's GN iteration since)
    {
        AvtRunParams* pr = nullptr;
        if (dev_alloc(c, &pr, 1)) return 1;
        fb.params = pr;
    }
    {   // the correspondence gate (avt_set_corr_gate): off, i.e. +inf for every part
        double* g2 = nullptr;
        if (dev_alloc(c, &g2, (size_t)num_parts) || dev_alloc(c, &fb.gated, (size_t)max_frames)) return 1;
        fb.gate2 = g2;
        c->gate_host.assign((size_t)num_parts, std::numeric_limits<double>::infinity());
        c->gate2_host = c->gate_host;
        AVT_HIP(hipMemcpyAsync(g2, c->gate2_host.data(), (size_t)num_parts * sizeof(double), hipMemcpyHostToDevice, c->stream));
        AVT_HIP(hipMemsetAsync(fb.gated, 0, (size_t)max_frames * sizeof(int), c->stream));
    }
    fb.spec_frames = std::min(max_frames, AVT_SPEC_FRAMES);
    if (dev_alloc(c, &fb.partial_spec, (size_t)fb.spec_frames * AVT_MAX_SPEC * AVT_G_MAX * 256) || dev_alloc(c, &fb.wmask_spec, (size_t)fb.spec_frames * AVT_MAX_SPEC * AVT_G_MAX) ||
        dev_alloc(c, &fb.prior_spec, (size_t)fb.spec_frames * AVT_MAX_SPEC * AVT_MAX_COMPS * AVT_PRIOR_STRIDE))
        return 1;
    fb.fsum = (long long*)cntsum;                                   // 8-byte aligned first
    fb.cnt = (int*)(cntsum + FV * 3 * sizeof(long long));
    AVT_HIP(hipMemsetAsync(fb.trace, 0, (size_t)max_frames * 64 * sizeof(double), c->stream));
    AVT_HIP(hipMemsetAsync(fb.ctl, 0, (size_t)max_frames * sizeof(AvtFrameCtl), c->stream));
    AVT_HIP(hipMemsetAsync(fb.ride_ctr, 0, (size_t)max_frames * sizeof(unsigned), c->stream));
    AVT_HIP(hipMemsetAsync(fb.fault, 0, (size_t)max_frames * sizeof(unsigned), c->stream));
    fb.ride_timeout = c->tun.ride_timeout_us * 100;      // wall_clock64() ticks at 100 MHz; 0 makes every wait that is not already satisfied fail (tests)
    fb.xcd_frames = c->tun.xcd_frames;
    AVT_HIP(hipMemsetAsync(fb.spec, 0, (size_t)max_frames * sizeof(AvtSpecCtl), c->stream));
    AVT_HIP(hipMemsetAsync(fb.part_cnt, 0, (size_t)max_frames * 2 * (AVT_MAX_PARTS + 1) * sizeof(int), c->stream));   // invariant of launch_bucket
    AVT_HIP(hipStreamSynchronize(c->stream));
    if (c->tun.debug) avt_eval_report_occupancy(dm.d);
    return 0;
}

int avt_ctx_create(int device, const avt_model* m, int num_parts, const int* part_map, int max_points, int max_frames, avt_ctx** out) {
    if (out) *out = nullptr;
    const int rc = avt_guard("avt_ctx_create", [&]() -> int { return ctx_create_impl(device, m, num_parts, part_map, max_points, max_frames, out); });
    if (rc != 0 && out && *out) {     // streams, events and every allocation made so far are released
        const std::string keep = avt_last_error();
        avt_ctx_destroy(*out);
        *out = nullptr;
        avt_set_error(keep);
    }
    return rc;
}

void avt_ctx_destroy(avt_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->host_pin) (void)hipHostFree(c->host_pin);
    // every device buffer (DevBuf members) goes with `delete`, after the events and the streams: the main stream has just been
    // drained and every side stream joins it, so nothing is queued on those buffers either way
    for (hipEvent_t e : c->event_pool) (void)hipEventDestroy(e);
    graph_drop_all(c);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->sub.ev_labels) (void)hipEventDestroy(c->sub.ev_labels);
    for (int i = 0; i < AVT_MAX_GROUPS - 1; ++i) {
        if (c->ev_join[i]) (void)hipEventDestroy(c->ev_join[i]);
        if (c->side[i]) (void)hipStreamDestroy(c->side[i]);
    }
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int avt_sync(avt_ctx* c) {
    return avt_guard("avt_sync", [&]() -> int {
        if (!c) { avt_set_error("avt_sync: null context"); return 1; }
        AVT_HIP(hipStreamSynchronize(c->stream));
        return 0;
    });
}

int avt_lbs_update(avt_ctx* c, int nframes, const double* w, const double* p, const double* R, double* cloud, double* joint_pos,
                   double* joint_trans) {
    return avt_guard("avt_lbs_update", [&]() -> int {
        if (!c || !w || !p || !R) { avt_set_error("avt_lbs_update: null argument"); return 1; }
        const AvtDims& d = c->dm.d;
        if (nframes <= 0 || nframes > c->fb.max_frames) { avt_set_error("avt_lbs_update: nframes out of range"); return 1; }
        AVT_HIP(hipSetDevice(c->device));
        c->frames_valid = c->state_valid = false;    // frame slots' posed clouds / skeleton scratch are overwritten
        LbsLaunch lbs;
        if (stage_pose(c, "avt_lbs_update", nframes, w, p, R, &lbs)) return 1;
        { ProfScope ps(c, AVT_K_LBS); launch_lbs(c, nframes, lbs); }
        if (check_launch("k_lbs")) return 1;
        return read_back(c, {{cloud, c->fb.cloud, (size_t)nframes * 3 * d.V * sizeof(double)}, {joint_pos, c->fb.jointpos, (size_t)nframes * 3 * d.J * sizeof(double)},
                             {joint_trans, c->fb.jointtrans, (size_t)nframes * 12 * d.J * sizeof(double)}});
    });
}

int avt_visibility(avt_ctx* c, const double* cloud, int enable, unsigned char* visible) {
    return avt_guard("avt_visibility", [&]() -> int {
        if (!c || !cloud || !visible) { avt_set_error("avt_visibility: null argument"); return 1; }
        const AvtDims& d = c->dm.d;
        AVT_HIP(hipSetDevice(c->device));
        c->frames_valid = c->state_valid = false;
        AVT_HIP(hipMemcpyAsync(c->fb.cloud, cloud, (size_t)3 * d.V * sizeof(double), hipMemcpyHostToDevice, c->stream));
        { ProfScope ps(c, AVT_K_VISIBILITY); launch_visibility(c, 1, enable); }
        if (check_launch("k_visibility")) return 1;
        return read_back(c, {{visible, c->fb.visible, (size_t)d.V}});
    });
}

int avt_nn(avt_ctx* c, const double* model_cloud, const unsigned char* visible, const double* data, const int* labels, int N, int* out) {
    return avt_guard("avt_nn", [&]() -> int {
        if (!c || !model_cloud || !visible || !data || !labels || !out) { avt_set_error("avt_nn: null argument"); return 1; }
        const AvtDims& d = c->dm.d;
        const int V = d.V;
        AVT_HIP(hipSetDevice(c->device));
        if (N == 0) return 0;
        const int offs[2] = {0, N};
        if (upload_frames(c, 1, data, labels, offs)) return 1;
        c->frames_valid = c->state_valid = false;    // frame slot 0 is scratch for this call
        c->nn_sums_frame0 = false;
        // part-sorted SoA copy of the model cloud
        std::vector<int> ppos(V);
        if (read_back(c, {{ppos.data(), c->dm.part_pos, (size_t)V * sizeof(int)}})) return 1;
        std::vector<double> px(V), py(V), pz(V);
        for (int v = 0; v < V; ++v) { px[ppos[v]] = model_cloud[3 * v]; py[ppos[v]] = model_cloud[3 * v + 1]; pz[ppos[v]] = model_cloud[3 * v + 2]; }
        AVT_HIP(hipMemcpyAsync(c->fb.pcx, px.data(), V * sizeof(double), hipMemcpyHostToDevice, c->stream));
        AVT_HIP(hipMemcpyAsync(c->fb.pcy, py.data(), V * sizeof(double), hipMemcpyHostToDevice, c->stream));
        AVT_HIP(hipMemcpyAsync(c->fb.pcz, pz.data(), V * sizeof(double), hipMemcpyHostToDevice, c->stream));
        AVT_HIP(hipMemcpyAsync(c->fb.visible, visible, (size_t)V, hipMemcpyHostToDevice, c->stream));
        // k_trim forms a match's distance from the cloud by vertex id (inside optimize() k_lbs wrote it beside the part-sorted copy)
        if (c->trim_on) AVT_HIP(hipMemcpyAsync(c->fb.cloud, model_cloud, (size_t)3 * V * sizeof(double), hipMemcpyHostToDevice, c->stream));
        std::unique_ptr<unsigned char[]> vs;
        if (c->tun.nn_force_vis) {      // the fused shape reads the flags in part-sorted order (inside optimize(): k_lbs / k_visibility keep them)
            vs.reset(new unsigned char[V]);
            for (int v = 0; v < V; ++v) vs[ppos[v]] = visible[v];
            AVT_HIP(hipMemcpyAsync(c->fb.vis_sorted, vs.get(), (size_t)V, hipMemcpyHostToDevice, c->stream));
        }
        AvtFrameCtl ctl;
        std::memset(&ctl, 0, sizeof(ctl));
        ctl.N = N;
        AVT_HIP(hipMemcpyAsync(c->fb.ctl, &ctl, sizeof(ctl), hipMemcpyHostToDevice, c->stream));
        { ProfScope ps(c, AVT_K_BUCKET); launch_bucket(c, 1, true); }
        { ProfScope ps(c, AVT_K_NN); launch_nn(c, 1); if (c->trim_on) launch_trim(c, 1); }
        c->trim_last = c->trim_on;
        if (check_launch("k_nn")) return 1;
        if (read_back(c, {{out, c->fb.corr, (size_t)N * sizeof(int)}})) return 1;
        c->nn_sums_frame0 = true;
        return 0;
    });
}

int avt_synth_render_frames(avt_ctx* c, int nframes, const double* w, const double* p, const double* R, double fx, double fy, double cx,
                            double cy, int width, int height, int* points_per_frame) {
    return avt_synth_render_frames_mode(c, nframes, w, p, R, fx, fy, cx, cy, width, height, AVT_RENDER_ZBUFFER, points_per_frame);
}

int avt_synth_render_frames_mode(avt_ctx* c, int nframes, const double* w, const double* p, const double* R, double fx, double fy, double cx,
                                 double cy, int width, int height, int mode, int* points_per_frame) {
    return avt_guard("avt_synth_render_frames", [&]() -> int {
        if (!c || !w || !p || !R || width <= 0 || height <= 0) { avt_set_error("avt_synth_render_frames: bad argument"); return 1; }
        if (mode != AVT_RENDER_ZBUFFER && mode != AVT_RENDER_PAINTER) { avt_set_error("avt_synth_render_frames: unknown mode"); return 1; }
        const bool painter = mode == AVT_RENDER_PAINTER;
        c->render_img_frames = 0;
        const AvtDims& d = c->dm.d;
        if (nframes <= 0 || nframes > c->fb.max_frames) { avt_set_error("avt_synth_render_frames: nframes out of range"); return 1; }
        AVT_HIP(hipSetDevice(c->device));
        // pose the ground-truth avatars (Avatar::update) for all frames
        LbsLaunch lbs;
        if (stage_pose(c, "avt_synth_render_frames", nframes, w, p, R, &lbs)) return 1;
        launch_lbs(c, nframes, lbs);
        // rasterise in chunks of frames (8 bytes of z-buffer key per pixel)
        const size_t npix = (size_t)width * height;
        const int chunk = std::max(1, std::min(nframes, (int)((256ull << 20) / (npix * (painter ? 21 : 9) + 64))));
        const int nb = (int)((npix + 255) / 256);
        // z-buffer keys, labels and block counts live in the context and only grow (no hipMalloc / hipFree per call)
        auto scratch = [&](auto& buf, size_t n) -> int {
            if (n <= buf.cap) return 0;
            AVT_HIP(hipStreamSynchronize(c->stream));     // what is queued on the old block drains before it goes
            return buf.reserve(n);
        };
        const size_t pix = npix * chunk, nface = (size_t)d.F * chunk;
        if (scratch(c->render_zkey, pix) || scratch(c->render_label, pix) || scratch(c->render_block, (size_t)nb * chunk)) return 1;
        if (painter && (scratch(c->render_mkey, pix) || scratch(c->render_depth, pix) || scratch(c->render_fkey, nface) || scratch(c->render_frank, nface) ||
                        scratch(c->render_fedge, nface)))
            return 1;
        int rc = 0;
        for (int f0 = 0; f0 < nframes && !rc; f0 += chunk) {
            c->fb.f0 = f0;
            const int nf = std::min(chunk, nframes - f0);
            if (painter)
                rc = avt_paint_enqueue(c, nf, c->dm.part_of_vertex, c->render_zkey, c->render_mkey, c->render_fkey, c->render_frank, c->render_fedge,
                                       c->render_depth, c->render_label, c->render_block, fx, fy, cx, cy, width, height);
            else
                rc = avt_render_enqueue(c, nf, c->dm.part_of_vertex, c->render_zkey, c->render_label, c->render_block, fx, fy, cx, cy, width, height);
        }
        c->fb.f0 = 0;
        if (rc) { avt_set_error("avt_synth_render_frames: render launch failed"); return 1; }
        std::vector<AvtFrameCtl> ctl(nframes);
        if (read_back(c, {{ctl.data(), c->fb.ctl, ctl.size() * sizeof(AvtFrameCtl)}})) return 1;
        c->frames_valid = c->state_valid = false;      // the rendered frames replace what was resident; they have no start state
        for (int f = 0; f < nframes; ++f)
            if (ctl[f].T > c->fb.max_points) { avt_set_error("avt_synth_render_frames: a rendered frame has more points than max_points_per_frame"); return 1; }
        if (set_resident_frames(c, nframes, [&](int f) { return ctl[f].N; })) return 1;
        if (points_per_frame) std::copy(c->frame_N.begin(), c->frame_N.end(), points_per_frame);
        // the render kernels wrote N into the working control blocks; the start copies follow (avt_state_reset)
        AVT_HIP(hipMemcpy2DAsync(&c->fb.ctl_start->N, sizeof(AvtFrameCtl), c->frame_N.data(), sizeof(int), sizeof(int), (size_t)nframes, hipMemcpyHostToDevice, c->stream));
        AVT_HIP(hipStreamSynchronize(c->stream));
        c->frames_valid = true;
        if (painter && nframes <= chunk) { c->render_img_frames = nframes; c->render_img_w = width; c->render_img_h = height; }
        return 0;
    });
}

int avt_synth_render_images(avt_ctx* c, int frame, float* depth, unsigned char* part_mask) {
    return avt_guard("avt_synth_render_images", [&]() -> int {
        if (!c) { avt_set_error("avt_synth_render_images: null context"); return 1; }
        if (c->render_img_frames == 0) {
            avt_set_error("avt_synth_render_images: no images retained (needs a preceding AVT_RENDER_PAINTER call whose frames fit one scratch chunk)");
            return 1;
        }
        if (frame < 0 || frame >= c->render_img_frames) { avt_set_error("avt_synth_render_images: frame out of range"); return 1; }
        const size_t npix = (size_t)c->render_img_w * c->render_img_h;
        return read_back(c, {{depth, c->render_depth + (size_t)frame * npix, npix * sizeof(float)}, {part_mask, c->render_label + (size_t)frame * npix, npix}});
    });
}

int avt_frames_download(avt_ctx* c, int frame, double* data_3xN, int* labels) {
    return avt_guard("avt_frames_download", [&]() -> int {
        if (!c || !c->frames_valid || frame < 0 || frame >= c->nframes) { avt_set_error("avt_frames_download: bad argument"); return 1; }
        const size_t N = c->frame_N[frame];
        return read_back(c, {{data_3xN, c->fb.data_raw + (size_t)frame * c->fb.max_points * 3, N * 3 * sizeof(double)}, {labels, c->fb.labels_raw + (size_t)frame * c->fb.max_points, N * sizeof(int)}});
    });
}

int avt_frames_upload(avt_ctx* c, int nframes, const double* data, const int* labels, const int* frame_offsets) {
    return avt_guard("avt_frames_upload", [&]() -> int {
        if (!c || !data || !labels || !frame_offsets) { avt_set_error("avt_frames_upload: null argument"); return 1; }
        AVT_HIP(hipSetDevice(c->device));
        if (upload_frames(c, nframes, data, labels, frame_offsets)) return 1;
        AVT_HIP(hipStreamSynchronize(c->stream));
        return 0;
    });
}

int avt_state_upload(avt_ctx* c, int nframes, const double* p, const double* q, const double* w) {
    return avt_guard("avt_state_upload", [&]() -> int {
        if (!c || !p || !q || !w) { avt_set_error("avt_state_upload: null argument"); return 1; }
        AVT_HIP(hipSetDevice(c->device));
        if (!c->frames_valid || nframes != c->nframes) { avt_set_error("state: nframes differs from the resident frames"); return 1; }
        std::vector<double> block((state_block_bytes(c, nframes) + 7) / 8);
        if (enqueue_start_states(c, nframes, block.data(), p, q, w)) return 1;
        AVT_HIP(hipStreamSynchronize(c->stream));  // the block goes out of scope
        c->state_valid = true;
        c->results_fresh = false;
        return 0;
    });
}

int avt_optimize_resident(avt_ctx* c, const avt_options* opt) {
    return avt_guard("avt_optimize_resident", [&]() -> int {
        if (!c || !opt) { avt_set_error("avt_optimize_resident: null argument"); return 1; }
        AVT_HIP(hipSetDevice(c->device));
        const int rc = run_optimize(c, opt);
        if (rc) c->results_fresh = false;      //  a call that failed left no result records
        return rc;
    });
}

int avt_optimize_resident_budgets(avt_ctx* c, const avt_options* opt, const int* icp_budget) {
    return avt_guard("avt_optimize_resident_budgets", [&]() -> int {
        if (!c || !opt || !icp_budget) { avt_set_error("avt_optimize_resident_budgets: null argument"); return 1; }
        AVT_HIP(hipSetDevice(c->device));
        if (check_optimize(c, opt)) return 1;
        const int nf = c->nframes;
        for (int f = 0; f < nf; ++f)
            if (icp_budget[f] < 0 || icp_budget[f] > opt->icp_iters) {
                char msg[160];
                snprintf(msg, sizeof msg, "avt_optimize_resident_budgets: frame %d has budget %d, outside [0, icp_iters = %d]", f, icp_budget[f], opt->icp_iters);
                avt_set_error(msg);
                return 1;
            }
        if (c->budget_hold.reserve((size_t)c->fb.max_frames * avt_budget_hold_doubles(c->dm.d)) || c->budget.reserve((size_t)c->fb.max_frames)) return 1;
        if (upload_when_changed(c, c->budget_host, icp_budget, (size_t)nf, false, [&](const int* b) -> int {
                for (int f0 = 0; f0 < nf; f0 += AVT_BUDGET_CHUNK) {
                    AvtBudgetChunk a;
                    a.f0 = f0;
                    a.n = std::min(AVT_BUDGET_CHUNK, nf - f0);
                    std::copy(b + f0, b + f0 + a.n, a.b);
                    launch_budget_set(c, c->budget, a);
                }
                return check_launch("k_budget_set");
            }))
            return 1;
        const int rc = run_optimize(c, opt, c->budget);
        c->results_fresh = false;      // the result records of the closing launch describe the frames before the held ones were put back
        return rc;
    });
}

int avt_state_upload_frames(avt_ctx* c, int count, const int* frames, const double* p, const double* q, const double* w) {
    return avt_guard("avt_state_upload_frames", [&]() -> int {
        if (!c || !frames || !p || !q || !w) { avt_set_error("avt_state_upload_frames: null argument"); return 1; }
        if (!c->frames_valid || !c->state_valid || c->nframes <= 0) { avt_set_error("avt_state_upload_frames: no resident state to update (avt_state_upload first)"); return 1; }
        const int nf = c->nframes;
        if (count <= 0 || count > nf) { avt_set_error("avt_state_upload_frames: count out of range"); return 1; }
        std::vector<char> seen(nf, 0);
        for (int i = 0; i < count; ++i) {
            if (frames[i] < 0 || frames[i] >= nf) { avt_set_error("avt_state_upload_frames: frame id out of range"); return 1; }
            if (seen[frames[i]]++) { avt_set_error("avt_state_upload_frames: a frame id is repeated"); return 1; }
        }
        AVT_HIP(hipSetDevice(c->device));
        const AvtDims& d = c->dm.d;
        for (int i = 0; i < count; ++i) {
            AvtStateInstall a;
            a.frame = frames[i];
            a.N = c->frame_N[frames[i]];
            pack_state_row(d, a.x, p, q, w, i);
            launch_state_install(c, a);
        }
        c->results_fresh = false;
        return check_launch("k_state_install");
    });
}

int avt_state_reset(avt_ctx* c) {
    return avt_guard("avt_state_reset", [&]() -> int {
        if (!c || c->nframes <= 0 || !c->state_valid) { avt_set_error("avt_state_reset: no state resident"); return 1; }
        AVT_HIP(hipSetDevice(c->device));
        launch_state_reset(c, c->nframes);
        c->results_fresh = false;
        return check_launch("k_state_reset");
    });
}

int avt_state_download(avt_ctx* c, double* p, double* q, double* w, avt_stats* st) {
    return avt_guard("avt_state_download", [&]() -> int {
        if (!c) { avt_set_error("avt_state_download: null context"); return 1; }
        const AvtDims& d = c->dm.d;
        const int nf = c->nframes;
        std::vector<double> xs((size_t)nf * 2 * d.xsize);
        std::vector<AvtFrameCtl> ctl(nf);
        std::vector<unsigned> fault(nf, 0u);
        if (read_back(c, {{xs.data(), c->fb.x, xs.size() * sizeof(double)}, {ctl.data(), c->fb.ctl, ctl.size() * sizeof(AvtFrameCtl)},
                          {fault.data(), c->fb.fault, fault.size() * sizeof(unsigned)}}))
            return 1;
        if (const int rc = check_device_faults(c, nf, [&](int f) { return fault[f]; })) return rc;
        for (int f = 0; f < nf; ++f) {
            unpack_state_row(d, &xs[((size_t)f * 2 + ctl[f].cur_slot) * d.xsize], p, q, w, f);
            if (!st) continue;
            st[f].initial_cost = ctl[f].cost_initial; st[f].final_cost = ctl[f].cost_cur; st[f].lambda = ctl[f].lambda;
            st[f].num_correspondences = ctl[f].T; st[f].matched_model_points = ctl[f].M;
            st[f].gn_iterations = ctl[f].gn_iterations; st[f].accepted_steps = ctl[f].accepted;
        }
        return 0;
    });
}

int avt_optimize_batch(avt_ctx* c, int nframes, const double* data, const int* labels, const int* frame_offsets, const avt_options* opt,
                       double* p, double* q, double* w, avt_stats* stats) {
    return avt_guard("avt_optimize_batch", [&]() -> int {
        if (!c || !data || !labels || !frame_offsets || !opt || !p || !q || !w) { avt_set_error("avt_optimize_batch: null argument"); return 1; }
        AVT_HIP(hipSetDevice(c->device));
        return optimize_host_to_host(c, nframes, data, labels, frame_offsets, opt, p, q, w, stats);
    });
}

int avt_optimize(avt_ctx* c, const double* data, const int* labels, int N, const avt_options* opt, double* p, double* q, double* w,
                 avt_stats* stats) {
    const int offs[2] = {0, N};
    return avt_optimize_batch(c, 1, data, labels, offs, opt, p, q, w, stats);
}

int avt_optimize_posed(avt_ctx* c, const double* data, const int* labels, int N, const avt_options* opt, double* p, double* q, double* w,
                       avt_stats* stats, double* cloud, double* joint_pos, double* joint_trans) {
    return avt_guard("avt_optimize_posed", [&]() -> int {
        if (!c || !data || !labels || !opt || !p || !q || !w) { avt_set_error("avt_optimize_posed: null argument"); return 1; }
        if (opt->icp_iters <= 0 && (cloud || joint_pos || joint_trans)) { avt_set_error("avt_optimize_posed: no ICP iteration, no closing update(): nothing posed to return"); return 1; }
        AVT_HIP(hipSetDevice(c->device));
        const int offs[2] = {0, N};
        return optimize_host_to_host(c, 1, data, labels, offs, opt, p, q, w, stats, cloud, joint_pos, joint_trans);
    });
}

int avt_get_correspondences(avt_ctx* c, int frame, int* out) {
    return avt_guard("avt_get_correspondences", [&]() -> int {
        if (!c || !out || frame < 0 || frame >= c->nframes) { avt_set_error("avt_get_correspondences: bad argument"); return 1; }
        return read_back(c, {{out, c->fb.corr + (size_t)frame * c->fb.max_points, (size_t)c->frame_N[frame] * sizeof(int)}});
    });
}

int avt_get_cloud(avt_ctx* c, int frame, double* cloud) {
    return avt_guard("avt_get_cloud", [&]() -> int {
        if (!c || !cloud || frame < 0 || frame >= c->fb.max_frames) { avt_set_error("avt_get_cloud: bad argument"); return 1; }
        return read_back(c, {{cloud, c->fb.cloud + (size_t)frame * 3 * c->dm.d.V, (size_t)3 * c->dm.d.V * sizeof(double)}});
    });
}

int avt_get_posed(avt_ctx* c, int frame, double* cloud, double* joint_pos, double* joint_trans) {
    return avt_guard("avt_get_posed", [&]() -> int {
        if (!c || frame < 0 || frame >= c->fb.max_frames) { avt_set_error("avt_get_posed: bad argument"); return 1; }
        const AvtDims& d = c->dm.d;
        return read_back(c, {{cloud, c->fb.cloud + (size_t)frame * 3 * d.V, (size_t)3 * d.V * sizeof(double)}, {joint_pos, c->fb.jointpos + (size_t)frame * 3 * d.J, (size_t)3 * d.J * sizeof(double)},
                             {joint_trans, c->fb.jointtrans + (size_t)frame * 12 * d.J, (size_t)12 * d.J * sizeof(double)}});
    });
}

int avt_get_normal_equations(avt_ctx* c, int frame, double* H, double* g, double* cost) {
    return avt_guard("avt_get_normal_equations", [&]() -> int {
        if (!c || frame < 0 || frame >= c->nframes) { avt_set_error("avt_get_normal_equations: bad argument"); return 1; }
        if (!c->frames_valid || !c->state_valid || c->ran_icp_iters <= 0) { avt_set_error("avt_get_normal_equations: no optimize call has run on the resident frames"); return 1; }
        const AvtDims& d = c->dm.d;
        AVT_HIP(hipSetDevice(c->device));
        // optimize() does not build the system of its last trial point (only that point's cost is needed): evaluate the data term
        // at the CURRENT point here - trial point := current point (SOLVE_INIT), one full evaluation, one reduction - with the
        // correspondences of the last ICP iteration.  The current point, its cost and the LM state are left untouched.
        const int G_keep = c->fb.G;
        c->fb.G = choose_G(c->nframes, 1, c->tun);
        c->fb.f0 = 0;
        c->cur_stream = c->stream;
        // the form of the data term: the one selected (AUTO: the one the last optimize() ran); what that form needs of the resident
        // correspondences - moments or matched-point records - is made here if the last optimize() ran the other form
        const bool want_mom = c->dm.d.mom_ok && (c->data_term == AVT_DATA_TERM_MOMENTS || (c->data_term == AVT_DATA_TERM_AUTO && c->last_run_moments));
        const int use_moments_keep = c->fb.use_moments;      // (restored below: plan_groups / avt_launch_shape read it)
        c->fb.use_moments = want_mom;
        launch_solve(c, c->nframes, SOLVE_INIT);
        if (want_mom) {
            if (!c->have_moments) { c->fb.const_used = (c->launch_maxN + 2047) / 2048; launch_moments(c, c->nframes); c->have_moments = true; }
            launch_assemble(c, c->nframes);
        } else {
            if (!c->have_records) { c->fb.const_used = (c->launch_maxN + 255) / 256; launch_records(c, c->nframes); c->have_records = true; }
            launch_eval(c, c->nframes, false);
            launch_reduce(c, c->nframes);
        }
        c->fb.G = G_keep;
        c->fb.use_moments = use_moments_keep;
        if (check_launch("avt_get_normal_equations")) return 1;
        AvtFrameCtl ctl;      // (first: its cur_slot says which of the frame's two systems is the trial point's)
        if (read_back(c, {{&ctl, c->fb.ctl + frame, sizeof(ctl)}})) return 1;
        std::vector<double> buf((size_t)d.HS * d.HS);
        if (read_back(c, {{buf.data(), c->fb.Hraw + ((size_t)frame * 2 + (1 - ctl.cur_slot)) * buf.size(), buf.size() * sizeof(double)}})) return 1;
        for (int r = 0; r < d.P; ++r) {
            if (H) for (int q = 0; q < d.P; ++q) H[(size_t)r * d.P + q] = buf[(size_t)r * d.HS + q];
            if (g) g[r] = buf[(size_t)d.P * d.HS + r];
        }
        if (cost) *cost = ctl.cost_cur;
        return 0;
    });
}

int avt_debug_mfma_count(avt_ctx* c, int frame, long long* eval_rows, long long* moments, long long* solve) {
    return avt_guard("avt_debug_mfma_count", [&]() -> int {
        if (!c || frame < 0 || frame >= c->nframes) { avt_set_error("avt_debug_mfma_count: bad argument"); return 1; }
        if (!c->frames_valid || c->ran_icp_iters <= 0) { avt_set_error("avt_debug_mfma_count: no optimize call has run on the resident frames"); return 1; }
        const AvtDims& d = c->dm.d;
        if (solve) *solve = avt_solve_mfma_count(d);
        if (moments) {
            *moments = -1;
            if (d.mom_ok) {
                std::vector<int> cnt(d.V);
                if (read_back(c, {{cnt.data(), c->fb.cnt + (size_t)frame * d.V, cnt.size() * sizeof(int)}})) return 1;
                *moments = avt_moments_mfma_count(c->model, cnt.data());
            }
        }
        if (eval_rows) {
            *eval_rows = -1;
            if (c->have_records && d.NT <= 6) {
                // k_records leaves one word per batch of 16 matched points: bits 0..23 = the live tile pairs (avt_eval.hip); k_eval runs the
                // 12 k-steps (48 rows / 4) of every live pair - the split pair's are dealt over the four waves, 12 in total all the same
                AvtFrameCtl ctl;      // (first: its M says how many batches there are)
                if (read_back(c, {{&ctl, c->fb.ctl + frame, sizeof(ctl)}})) return 1;
                const int nb = (ctl.M + AVT_EVAL_PTS - 1) / AVT_EVAL_PTS;
                std::vector<int> bm(std::max(nb, 1));
                if (read_back(c, {{bm.data(), c->fb.bmask + (size_t)frame * d.nb_max, (size_t)nb * sizeof(int)}})) return 1;
                long long n = 0;
                for (int b = 0; b < nb; ++b) n += 12ll * __builtin_popcount((unsigned)bm[b] & 0xffffffu);
                *eval_rows = n;
            }
        }
        return 0;
    });
}

int avt_debug_nn_sums(avt_ctx* c, int frame, int* cnt, long long* fsum, double* centre) {
    return avt_guard("avt_debug_nn_sums", [&]() -> int {
        if (!c || frame < 0 || frame >= c->fb.max_frames) { avt_set_error("avt_debug_nn_sums: bad argument"); return 1; }
        if (last_search_left(c, "avt_debug_nn_sums", frame)) return 1;
        const size_t V = c->dm.d.V;
        AvtFrameCtl ctl;
        if (read_back(c, {{cnt, c->fb.cnt + (size_t)frame * V, V * sizeof(int)}, {fsum, c->fb.fsum + (size_t)frame * 3 * V, 3 * V * sizeof(long long)}, {&ctl, c->fb.ctl + frame, sizeof(ctl)}}))
            return 1;
        if (centre) for (int k = 0; k < 3; ++k) centre[k] = ctl.centre[k];
        return 0;
    });
}

int avt_ctx_get_tuning(avt_ctx* c, avt_tuning* out) {
    return avt_guard("avt_ctx_get_tuning", [&]() -> int {
        if (!c || !out) { avt_set_error("avt_ctx_get_tuning: null argument"); return 1; }
        *out = c->tun;
        return 0;
    });
}

int avt_ctx_set_tuning(avt_ctx* c, const avt_tuning* t) {
    return avt_guard("avt_ctx_set_tuning", [&]() -> int {
        if (!c || !t) { avt_set_error("avt_ctx_set_tuning: null argument"); return 1; }
        if (validate_tuning(*t)) return 1;
        AVT_HIP(hipSetDevice(c->device));
        AVT_HIP(hipStreamSynchronize(c->stream));
        graph_drop_all(c);      // the launch sequences captured so far were made with the old knobs
        c->tun = *t;
        c->vis_frame_min = avt_visibility_frame_lds(c->dm.d) <= 150 * 1024 ? c->tun.vis_frame_min : 0;
        c->fb.ride_timeout = c->tun.ride_timeout_us * 100;
        c->fb.xcd_frames = c->tun.xcd_frames;
        return 0;
    });
}

int avt_set_data_term(avt_ctx* c, int form) {
    return avt_guard("avt_set_data_term", [&]() -> int {
        if (!c || (form != AVT_DATA_TERM_ROWS && form != AVT_DATA_TERM_MOMENTS && form != AVT_DATA_TERM_AUTO)) { avt_set_error("avt_set_data_term: bad argument"); return 1; }
        if (form == AVT_DATA_TERM_MOMENTS && !c->dm.d.mom_ok) { avt_set_error("avt_set_data_term: this model has no moment form (" + c->mom_reason + ")"); return 1; }
        c->data_term = form;
        return 0;
    });
}

int avt_get_data_term(avt_ctx* c) { return c ? c->data_term : -1; }

int avt_set_occlusion_render(avt_ctx* c, int width, int height, float fx, float fy, float cx, float cy) {
    return avt_guard("avt_set_occlusion_render", [&]() -> int {
        if (!c) { avt_set_error("avt_set_occlusion_render: null context"); return 1; }
        if (width != 0 && (width < 0 || height <= 0 || width >= 65536 || (long long)width * height >= (1ll << 31))) {
            avt_set_error("avt_set_occlusion_render: bad image size (0 < width < 65536, height > 0, width x height < 2^31; width 0 turns the mode off)");
            return 1;
        }
        AVT_HIP(hipSetDevice(c->device));
        // the scratch of the new size first, beside the old one: a refused call leaves the previous setting in force
        DevBuf<int> faces, order, rank; DevBuf<float> fkey, proj; DevBuf<unsigned char> front;
        if (width > 0) {
            const size_t nf = (size_t)c->fb.max_frames, F = (size_t)std::max(c->dm.d.F, 1), V = (size_t)c->dm.d.V;
            if (faces.reserve(nf * width * height) || order.reserve(nf * F) || rank.reserve(nf * F) || fkey.reserve(nf * F) || proj.reserve(nf * 2 * V) ||
                front.reserve(nf * F)) {
                (void)hipGetLastError();
                avt_set_error(std::string("avt_set_occlusion_render: the device cannot hold the face images of every frame slot (") + avt_last_error() + ")");
                return 1;
            }
        }
        AVT_HIP(hipStreamSynchronize(c->stream));      // nothing queued reads the old scratch any more
        graph_drop_all(c);      // the launch sequences captured so far hold the old rule and the old scratch
        c->occ_faces = std::move(faces); c->occ_order = std::move(order); c->occ_rank = std::move(rank);
        c->occ_fkey = std::move(fkey); c->occ_proj = std::move(proj); c->occ_front = std::move(front);
        c->occ_w = width; c->occ_h = width > 0 ? height : 0;
        c->occ_fx = fx; c->occ_fy = fy; c->occ_cx = cx; c->occ_cy = cy;
        return 0;
    });
}

int avt_set_corr_gate(avt_ctx* c, int n, const double* max_dist) {
    return avt_guard("avt_set_corr_gate", [&]() -> int {
        if (!c) { avt_set_error("avt_set_corr_gate: null context"); return 1; }
        const int np = c->dm.d.num_parts;
        if (!max_dist) n = 0;
        if (check_per_part("avt_set_corr_gate", n, np, [&](int i) -> std::string {
                if (i < 0 || max_dist[i] >= 0.0) return "";      // (a NaN fails every comparison)
                return "value " + std::to_string(i) + " is negative or not a number (each of the 1 or num_parts = " + std::to_string(np) + " gates is a distance >= 0, +inf allowed)";
            }))
            return 1;
        c->gate_host = per_part(n, np, max_dist, std::numeric_limits<double>::infinity());
        std::vector<double> g2((size_t)np);
        for (int q = 0; q < np; ++q) g2[(size_t)q] = c->gate_host[(size_t)q] * c->gate_host[(size_t)q];
        return upload_when_changed(c, c->gate2_host, g2.data(), g2.size(), true, [&](const double* src) -> int {
            AVT_HIP(hipMemcpyAsync((void*)c->fb.gate2, src, (size_t)np * sizeof(double), hipMemcpyHostToDevice, c->stream));
            return 0;
        });
    });
}

int avt_get_corr_gate(avt_ctx* c, double* max_dist) {
    return avt_guard("avt_get_corr_gate", [&]() -> int {
        if (!c || !max_dist) { avt_set_error("avt_get_corr_gate: null argument"); return 1; }
        std::copy(c->gate_host.begin(), c->gate_host.end(), max_dist);
        return 0;
    });
}

int avt_get_gated(avt_ctx* c, int frame, int* gated) {
    return avt_guard("avt_get_gated", [&]() -> int {
        if (!c || !gated || frame < 0 || frame >= c->fb.max_frames) { avt_set_error("avt_get_gated: bad argument"); return 1; }
        if (last_search_left(c, "avt_get_gated", frame)) return 1;
        return read_back(c, {{gated, c->fb.gated + frame, sizeof(int)}});
    });
}

// ---- trimmed ICP (avt_trim.hip) ----
int avt_set_corr_trim(avt_ctx* c, int n, const double* quantile, const double* factor, const double* floor_dist, int min_matches) {
    return avt_guard("avt_set_corr_trim", [&]() -> int {
        if (!c) { avt_set_error("avt_set_corr_trim: null context"); return 1; }
        const int np = c->dm.d.num_parts;
        const double inf = std::numeric_limits<double>::infinity();
        if (!quantile || !factor || !floor_dist) {
            if (n != 0 && (quantile || factor || floor_dist)) { avt_set_error("avt_set_corr_trim: quantile, factor and floor_dist go together (all NULL: off)"); return 1; }
            n = 0;
        }
        if (check_per_part("avt_set_corr_trim", n, np, [&](int i) -> std::string {
                if (i < 0) return n > 0 && min_matches < 1 ? "min_matches = " + std::to_string(min_matches) + "; >= 1 wanted (values are per part: 1 or num_parts = " + std::to_string(np) + ")" : "";
                const double r = quantile[i], k = factor[i], fl = floor_dist[i];
                // (a NaN fails every comparison)
                if (r > 0.0 && r <= 1.0 && k >= 0.0 && (k == inf || k * k < inf) && fl >= 0.0 && fl < inf) return "";
                return "value " + std::to_string(i) + " of the 1 or num_parts = " + std::to_string(np) +
                       " is refused (quantile in (0, 1]; factor >= 0 with a finite square, or +inf; floor_dist >= 0 and finite; no NaN)";
            }))
            return 1;
        const std::vector<double> rho = per_part(n, np, quantile, 1.0), kap = per_part(n, np, factor, inf), flo = per_part(n, np, floor_dist, 0.0);
        std::vector<double> set((size_t)3 * np + 1);
        bool on = false;
        for (int q = 0; q < np; ++q) {
            set[(size_t)q] = rho[(size_t)q];
            set[(size_t)np + q] = kap[(size_t)q] * kap[(size_t)q];
            set[(size_t)2 * np + q] = flo[(size_t)q] * flo[(size_t)q];
            on = on || kap[(size_t)q] < inf;
        }
        const int mm = n > 0 ? min_matches : 1;
        set[(size_t)3 * np] = (double)mm;
        if (on) {
            AVT_HIP(hipSetDevice(c->device));
            if (!c->trim_set.p) {      // the first time trimming is enabled
                const size_t fn = (size_t)c->fb.max_frames * np;
                if (c->trim_set.reserve(set.size()) || c->trim_thr.reserve(fn) || c->trim_count.reserve(fn)) return 1;
                c->trim_set_host.clear();
            }
            if (upload_when_changed(c, c->trim_set_host, set.data(), set.size(), true, [&](const double* src) -> int {
                    AVT_HIP(hipMemcpyAsync(c->trim_set.p, src, set.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
                    return 0;
                }))
                return 1;
        }
        c->trim_rho = rho; c->trim_kappa = kap; c->trim_floor = flo; c->trim_min_matches = mm; c->trim_on = on;
        return 0;
    });
}

int avt_get_corr_trim(avt_ctx* c, double* quantile, double* factor, double* floor_dist, int* min_matches) {
    return avt_guard("avt_get_corr_trim", [&]() -> int {
        if (!c) { avt_set_error("avt_get_corr_trim: null context"); return 1; }
        const size_t np = (size_t)c->dm.d.num_parts;
        const bool never = c->trim_rho.empty();      // never set: off
        for (size_t q = 0; q < np; ++q) {
            if (quantile) quantile[q] = never ? 1.0 : c->trim_rho[q];
            if (factor) factor[q] = never ? std::numeric_limits<double>::infinity() : c->trim_kappa[q];
            if (floor_dist) floor_dist[q] = never ? 0.0 : c->trim_floor[q];
        }
        if (min_matches) *min_matches = c->trim_min_matches;
        return 0;
    });
}

// (where the counts of avt_get_gated are valid, those of the trim are)
int avt_get_trimmed(avt_ctx* c, int frame, int* total, int* per_part) {
    return avt_guard("avt_get_trimmed", [&]() -> int {
        if (!c || !total) { avt_set_error("avt_get_trimmed: null argument"); return 1; }
        if (frame < 0 || frame >= c->fb.max_frames) { avt_set_error("avt_get_trimmed: bad argument"); return 1; }
        if (last_search_left(c, "avt_get_trimmed", frame)) return 1;
        const int np = c->dm.d.num_parts;
        std::vector<int> n((size_t)np, 0);
        // (a search without trimming dropped nothing, whatever an earlier one left in the block)
        if (c->trim_last && read_back(c, {{n.data(), c->trim_count.p + (size_t)frame * np, (size_t)np * sizeof(int)}})) return 1;
        *total = 0;
        for (int q = 0; q < np; ++q) { *total += n[(size_t)q]; if (per_part) per_part[q] = n[(size_t)q]; }
        return 0;
    });
}

int avt_get_trim_thresholds(avt_ctx* c, int frame, double* T) {
    return avt_guard("avt_get_trim_thresholds", [&]() -> int {
        if (!c || !T) { avt_set_error("avt_get_trim_thresholds: null argument"); return 1; }
        if (frame < 0 || frame >= c->fb.max_frames) { avt_set_error("avt_get_trim_thresholds: bad argument"); return 1; }
        if (last_search_left(c, "avt_get_trim_thresholds", frame)) return 1;
        const int np = c->dm.d.num_parts;
        if (!c->trim_last) { std::fill(T, T + np, std::numeric_limits<double>::infinity()); return 0; }
        return read_back(c, {{T, c->trim_thr.p + (size_t)frame * np, (size_t)np * sizeof(double)}});
    });
}

int avt_get_visibility(avt_ctx* c, int frame, unsigned char* visible) {
    return avt_guard("avt_get_visibility", [&]() -> int {
        if (!c || !visible || frame < 0 || frame >= c->nframes) { avt_set_error("avt_get_visibility: bad argument"); return 1; }
        if (!c->frames_valid || c->ran_icp_iters <= 0) { avt_set_error("avt_get_visibility: no optimize call with an ICP iteration has run on the resident frames"); return 1; }
        return read_back(c, {{visible, c->fb.visible + (size_t)frame * c->dm.d.V, (size_t)c->dm.d.V}});
    });
}

int avt_debug_trace(avt_ctx* c, int frame, double* out64) {
    return avt_guard("avt_debug_trace", [&]() -> int {
        if (!c || !out64 || frame < 0 || frame >= c->fb.max_frames) { avt_set_error("avt_debug_trace: bad argument"); return 1; }
        return read_back(c, {{out64, c->fb.trace + (size_t)frame * 64, 64 * sizeof(double)}});
    });
}

int avt_launch_shape(avt_ctx* c, int* groups, int* frames_per_group, int* eval_workgroups_per_frame) {
    return avt_guard("avt_launch_shape", [&]() -> int {
        if (!c || c->nframes <= 0) { avt_set_error("avt_launch_shape: no frames resident"); return 1; }
        const int use_moments_keep = c->fb.use_moments;
        c->fb.use_moments = choose_moments(c, c->nframes);      // the shape of the form the next optimize() will choose, whatever ran last
        const int ng = plan_groups(c, c->nframes), nfg = (c->nframes + ng - 1) / ng;
        c->fb.use_moments = use_moments_keep;
        if (groups) *groups = ng;
        if (frames_per_group) *frames_per_group = nfg;
        if (eval_workgroups_per_frame) *eval_workgroups_per_frame = choose_G(nfg, ng, c->tun);
        return 0;
    });
}

int avt_profile_begin(avt_ctx* c) {
    return avt_guard("avt_profile_begin", [&]() -> int {
        if (!c) { avt_set_error("avt_profile_begin: null context"); return 1; }
        c->profiling = true;
        c->prof_events.clear();
        c->event_pool_used = 0;
        return 0;
    });
}

int avt_profile_select(avt_ctx* c, unsigned mask) {
    return avt_guard("avt_profile_select", [&]() -> int {
        if (!c) { avt_set_error("avt_profile_select: null context"); return 1; }
        c->prof_mask = mask;
        return 0;
    });
}

int avt_profile_end(avt_ctx* c, avt_profile* out) {
    return avt_guard("avt_profile_end", [&]() -> int {
        if (!c || !out) { avt_set_error("avt_profile_end: null argument"); return 1; }
        AVT_HIP(hipSetDevice(c->device));
        AVT_HIP(hipStreamSynchronize(c->stream));
        std::memset(out, 0, sizeof(*out));
        for (auto& rec : c->prof_events) {
            float ms = 0.f;
            AVT_HIP(hipEventElapsedTime(&ms, rec.second.first, rec.second.second));
            out->ms[rec.first] += ms;
            out->launches[rec.first] += 1;
        }
        c->profiling = false;
        c->prof_events.clear();
        c->event_pool_used = 0;
        return 0;
    });
}

}  // extern "C"
