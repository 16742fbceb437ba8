// avt_rtree_train.cpp — host driver of the forest trainer (include/avt_rtree_train.h): image ingestion, the level loop with
// the leaf rules of trainFromNode (RTree.cpp:2501-2647), the renumbering into the reference's depth-first order, and
// trainTransfer's normalisation (:3408-3419).  The kernels are in avt_rtree_train.hip.
#include "avt_rtree_train.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <exception>
#include <vector>

#include "avt_internal.h"

#define TR_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { avt_set_error(std::string(#x) + ": " + hipGetErrorString(e_)); return 1; } } while (0)

namespace {

// a device buffer that grows by doubling and keeps its contents
template <class T>
struct DevVec {
    T* p = nullptr;
    size_t cap = 0;
    int reserve(size_t n, size_t keep, hipStream_t s) {
        if (n <= cap) return 0;
        size_t nc = std::max(n, 2 * cap);
        T* q = nullptr;
        TR_HIP(hipMalloc((void**)&q, nc * sizeof(T)));
        if (keep) TR_HIP(hipMemcpyAsync(q, p, keep * sizeof(T), hipMemcpyDeviceToDevice, s));
        TR_HIP(hipStreamSynchronize(s));
        if (p) (void)hipFree(p);
        p = q; cap = nc;
        return 0;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

struct Samples {
    DevVec<int> img, xy;
    DevVec<float> d;
    DevVec<unsigned char> lab;
    int reserve(size_t n, size_t keep, hipStream_t s) { return img.reserve(n, keep, s) || xy.reserve(n, keep, s) || d.reserve(n, keep, s) || lab.reserve(n, keep, s); }
    RtSamples dev() const { return RtSamples{img.p, xy.p, d.p, lab.p}; }
    void release() { img.release(); xy.release(); d.release(); lab.release(); }
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
    DevVec<RtImg> d_imgs;
    DevVec<float> store;              // crops
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
    float* d_depth = nullptr;
    unsigned char* d_mask = nullptr;
    int *d_scan = nullptr, *d_scratch = nullptr;
    long long* d_off = nullptr;
    int rc = 0;
    auto fail = [&](const std::string& what) { avt_set_error("avt_rtree_trainer_add_images: " + what); rc = 1; };
    do {
        if (hipMalloc((void**)&d_depth, n * npix * sizeof(float)) != hipSuccess || hipMalloc((void**)&d_mask, n * npix) != hipSuccess ||
            hipMalloc((void**)&d_scan, (size_t)n * 7 * sizeof(int)) != hipSuccess || hipMalloc((void**)&d_scratch, n * npix * sizeof(int)) != hipSuccess ||
            hipMalloc((void**)&d_off, (size_t)n * sizeof(long long)) != hipSuccess) { fail("out of device memory"); break; }
        if (hipMemcpyAsync(d_depth, depth, n * npix * sizeof(float), kind, st) != hipSuccess ||
            hipMemcpyAsync(d_mask, mask, n * npix, kind, st) != hipSuccess) { fail("image copy failed"); break; }
        if (rt_launch_img_scan(st, d_depth, d_mask, n, rows, cols, d_scan)) { fail("kernel launch failed"); break; }
        std::vector<int> scan((size_t)n * 7);
        if (hipMemcpyAsync(scan.data(), d_scan, scan.size() * sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess) { fail("scan failed"); break; }
        bool bad_label = false, bad_depth = false;
        for (int i = 0; i < n; ++i) { bad_label |= scan[7 * (size_t)i + 5] >= tr->p.num_parts; bad_depth |= scan[7 * (size_t)i + 6] != 0; }
        if (bad_label) { fail("a part-mask label is >= num_parts (and not 255)"); break; }
        if (bad_depth) { fail("depth must be finite and >= 0"); break; }
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
        if (tr->store.reserve((size_t)(tr->store_used + add_pix) + 1, (size_t)tr->store_used, st) ||
            tr->d_imgs.reserve(tr->imgs.size() + n, tr->imgs.size(), st) || tr->s.reserve((size_t)(tr->n_samples + add_s) + 1, (size_t)tr->n_samples, st)) {
            rc = 1;
            break;
        }
        if (hipMemcpyAsync(tr->d_imgs.p + base, bi.data(), n * sizeof(RtImg), hipMemcpyHostToDevice, st) != hipSuccess ||
            hipMemcpyAsync(d_off, off.data(), n * sizeof(long long), hipMemcpyHostToDevice, st) != hipSuccess) { fail("upload failed"); break; }
        if (rt_launch_crop(st, d_depth, n, rows, cols, tr->d_imgs.p + base, tr->store.p) ||
            rt_launch_select(st, d_depth, d_mask, n, rows, cols, tr->p.num_points_per_image, tr->p.seed, base, d_off, d_scratch, tr->s.dev())) {
            fail("kernel launch failed");
            break;
        }
        if (hipStreamSynchronize(st) != hipSuccess) { fail("stream failed"); break; }   // bi / off live on this frame
        tr->imgs.insert(tr->imgs.end(), bi.begin(), bi.end());
        tr->store_used += add_pix;
        tr->n_samples += add_s;
    } while (false);
    if (d_depth) (void)hipFree(d_depth);
    if (d_mask) (void)hipFree(d_mask);
    if (d_scan) (void)hipFree(d_scan);
    if (d_scratch) (void)hipFree(d_scratch);
    if (d_off) (void)hipFree(d_off);
    return rc;
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
    DevVec<RtNode> d_nodes;
    DevVec<int> d_counts, d_list;
    DevVec<RtChunk> d_chunks;
    DevVec<RtRes> d_res;
    struct Guard {
        Samples *a, *b; DevVec<RtNode>* n; DevVec<int>*c, *l; DevVec<RtChunk>* ch; DevVec<RtRes>* r;
        ~Guard() { a->release(); b->release(); n->release(); c->release(); l->release(); ch->release(); r->release(); }
    } guard{&a, &b, &d_nodes, &d_counts, &d_list, &d_chunks, &d_res};
    if (a.reserve((size_t)N, 0, st) || b.reserve((size_t)N, 0, st)) return 1;
    TR_HIP(hipMemcpyAsync(a.img.p, tr->s.img.p, N * sizeof(int), hipMemcpyDeviceToDevice, st));
    TR_HIP(hipMemcpyAsync(a.xy.p, tr->s.xy.p, N * sizeof(int), hipMemcpyDeviceToDevice, st));
    TR_HIP(hipMemcpyAsync(a.d.p, tr->s.d.p, N * sizeof(float), hipMemcpyDeviceToDevice, st));
    TR_HIP(hipMemcpyAsync(a.lab.p, tr->s.lab.p, N, hipMemcpyDeviceToDevice, st));

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
        if (d_nodes.reserve(M, 0, st) || d_counts.reserve((size_t)M * P, 0, st) || d_res.reserve(M, 0, st) || d_list.reserve(list.size() + 1, 0, st) ||
            d_chunks.reserve((size_t)nl * nch_l + (size_t)ns * nch_s + 1, 0, st))
            return 1;
        TR_HIP(hipMemcpyAsync(d_nodes.p, level.data(), M * sizeof(RtNode), hipMemcpyHostToDevice, st));
        if (!list.empty()) TR_HIP(hipMemcpyAsync(d_list.p, list.data(), list.size() * sizeof(int), hipMemcpyHostToDevice, st));
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
        TR_HIP(hipMemcpyAsync(res.data(), d_res.p, M * sizeof(RtRes), hipMemcpyDeviceToHost, st));
        TR_HIP(hipMemcpyAsync(counts.data(), d_counts.p, counts.size() * sizeof(int), hipMemcpyDeviceToHost, st));
        TR_HIP(hipStreamSynchronize(st));                 // the one wait of the level
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
    TR_HIP(hipSetDevice(rt->device));
    if (!rt->d_tcount) {
        TR_HIP(hipMalloc((void**)&rt->d_tcount, ncnt * sizeof(unsigned long long)));
        TR_HIP(hipMemsetAsync(rt->d_tcount, 0, ncnt * sizeof(unsigned long long), rt->stream));
    }
    const size_t npix = (size_t)rows * cols;
    const int batch = (int)std::max<size_t>(1, std::min<size_t>(n, ((size_t)256 << 20) / (npix * 5)));
    float* d_depth = nullptr;
    unsigned char* d_mask = nullptr;
    unsigned long long* d_cnt = nullptr;
    int* d_bad = nullptr;
    int rc = 0, bad = 0;
    do {
        if (hipMalloc((void**)&d_depth, batch * npix * sizeof(float)) != hipSuccess || hipMalloc((void**)&d_mask, batch * npix) != hipSuccess ||
            hipMalloc((void**)&d_cnt, ncnt * sizeof(unsigned long long)) != hipSuccess || hipMalloc((void**)&d_bad, sizeof(int)) != hipSuccess ||
            hipMemsetAsync(d_cnt, 0, ncnt * sizeof(unsigned long long), rt->stream) != hipSuccess ||
            hipMemsetAsync(d_bad, 0, sizeof(int), rt->stream) != hipSuccess) { rc = 1; break; }
        for (int i0 = 0; i0 < n && !rc; i0 += batch) {
            const int k = std::min(batch, n - i0);
            if (hipMemcpyAsync(d_depth, depth + i0 * npix, k * npix * sizeof(float), kind, rt->stream) != hipSuccess ||
                hipMemcpyAsync(d_mask, mask + i0 * npix, k * npix, kind, rt->stream) != hipSuccess ||
                rt_launch_transfer(rt->stream, rt->d_nodes, d_depth, d_mask, k, rows, cols, P, d_cnt, d_bad) ||
                hipStreamSynchronize(rt->stream) != hipSuccess)   // the next batch goes into the same buffers
                rc = 1;
        }
        if (rc) break;
        if (hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, rt->stream) != hipSuccess || hipStreamSynchronize(rt->stream) != hipSuccess) {
            rc = 1;
            break;
        }
        if (bad) break;
        // the batch is good: add its integer counts to those kept since the last finish
        std::vector<unsigned long long> add(ncnt), acc(ncnt);
        if (hipMemcpyAsync(add.data(), d_cnt, ncnt * sizeof(unsigned long long), hipMemcpyDeviceToHost, rt->stream) != hipSuccess ||
            hipMemcpyAsync(acc.data(), rt->d_tcount, ncnt * sizeof(unsigned long long), hipMemcpyDeviceToHost, rt->stream) != hipSuccess ||
            hipStreamSynchronize(rt->stream) != hipSuccess) { rc = 1; break; }
        for (size_t i = 0; i < ncnt; ++i) acc[i] += add[i];
        if (hipMemcpyAsync(rt->d_tcount, acc.data(), ncnt * sizeof(unsigned long long), hipMemcpyHostToDevice, rt->stream) != hipSuccess ||
            hipStreamSynchronize(rt->stream) != hipSuccess) rc = 1;
    } while (false);
    if (d_depth) (void)hipFree(d_depth);
    if (d_mask) (void)hipFree(d_mask);
    if (d_cnt) (void)hipFree(d_cnt);
    if (d_bad) (void)hipFree(d_bad);
    if (rc) { avt_set_error(std::string(who) + ": device call failed"); return 1; }
    if (bad) { avt_set_error(std::string(who) + ": a part-mask label is >= num_parts (and not 255); the batch's counts were dropped"); return 1; }
    return 0;
}

// count / sum for every leaf with a count (RTree.cpp:3408-3419), the counts start over
int transfer_finish(avt_rtree* rt, int* n_unvisited) {
    const int P = rt->num_parts, nl = (int)rt->leaf_best.size();
    int unvisited = nl;
    if (rt->d_tcount) {
        TR_HIP(hipSetDevice(rt->device));
        const size_t ncnt = std::max<size_t>(1, (size_t)nl * P);
        std::vector<unsigned long long> cnt(ncnt);
        TR_HIP(hipMemcpyAsync(cnt.data(), rt->d_tcount, ncnt * sizeof(unsigned long long), hipMemcpyDeviceToHost, rt->stream));
        TR_HIP(hipStreamSynchronize(rt->stream));
        (void)hipFree(rt->d_tcount);
        rt->d_tcount = nullptr;
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
    RtNode* d_node = nullptr;
    int *d_counts = nullptr, *d_list = nullptr, *d_hist = nullptr;
    float* d_mm = nullptr;
    RtChunk* d_ch = nullptr;
    int rc = 0;
    const size_t nh = (size_t)nf * P * T;
    if (hipMalloc((void**)&d_node, sizeof(RtNode)) != hipSuccess || hipMalloc((void**)&d_counts, P * sizeof(int)) != hipSuccess ||
        hipMalloc((void**)&d_list, sizeof(int)) != hipSuccess || hipMalloc((void**)&d_hist, nh * sizeof(int)) != hipSuccess ||
        hipMalloc((void**)&d_mm, 2 * (size_t)nf * sizeof(float)) != hipSuccess || hipMalloc((void**)&d_ch, nf * sizeof(RtChunk)) != hipSuccess ||
        hipMemcpyAsync(d_node, &root, sizeof(RtNode), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(d_list, &zero, sizeof(int), hipMemcpyHostToDevice, st) != hipSuccess ||
        rt_launch_count(st, d_node, 1, tr->s.lab.p, P, d_counts) ||
        rt_launch_search(st, tr->n_samples >= 2048, d_list, 1, nf, 1, d_node, d_counts, tr->s.dev(), tr->d_imgs.p, tr->store.p, args, d_ch, d_hist, d_mm) ||
        hipMemcpyAsync(hist, d_hist, nh * sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
        (minmax && hipMemcpyAsync(minmax, d_mm, 2 * (size_t)nf * sizeof(float), hipMemcpyDeviceToHost, st) != hipSuccess) ||
        hipStreamSynchronize(st) != hipSuccess)
        rc = 1;
    for (void* q : {(void*)d_node, (void*)d_counts, (void*)d_list, (void*)d_hist, (void*)d_mm, (void*)d_ch})
        if (q) (void)hipFree(q);
    if (rc) avt_set_error("avt_rtree_trainer_root_histograms: device call failed");
    return rc;
}

}  // namespace

extern "C" {

int avt_rtree_trainer_create(int device, const avt_rtree_train_params* p, avt_rtree_trainer** out) {
    try {
        if (!p || !out || p->num_parts < 1 || p->num_parts > 127 || p->num_points_per_image < 1 || p->num_features < 1 ||
            !(p->max_probe_offset > 0.5f) || std::isinf(p->max_probe_offset) || p->min_samples < 0 || p->max_tree_depth < 1 ||
            p->max_tree_depth > AVT_RTREE_TRAIN_MAX_DEPTH || p->min_samples_per_feature < 1 || (long long)p->num_parts * p->min_samples_per_feature > 8192) {
            avt_set_error("avt_rtree_trainer_create: bad parameters (1 <= num_parts <= 127, points / features / T >= 1, max_probe_offset > 0.5, "
                          "min_samples >= 0, 1 <= max_tree_depth <= 64, num_parts x T <= 8192)");
            return 1;
        }
        TR_HIP(hipSetDevice(device));
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
    } catch (const std::exception& e) { avt_set_error(std::string("avt_rtree_trainer_create: ") + e.what()); return 1; }
    catch (...) { avt_set_error("avt_rtree_trainer_create: unknown exception"); return 1; }
}

void avt_rtree_trainer_destroy(avt_rtree_trainer* tr) {
    if (!tr) return;
    (void)hipSetDevice(tr->device);
    if (tr->stream) (void)hipStreamSynchronize(tr->stream);
    tr->d_imgs.release();
    tr->store.release();
    tr->s.release();
    if (tr->stream) (void)hipStreamDestroy(tr->stream);
    delete tr;
}

int avt_rtree_trainer_add_images(avt_rtree_trainer* tr, int n, int rows, int cols, const float* depth, const unsigned char* mask) {
    try {
        if (check_args(tr, n, rows, cols, depth, mask, "avt_rtree_trainer_add_images")) return 1;
        TR_HIP(hipSetDevice(tr->device));
        // batches of at most ~512 MB of temporaries; image indices and samples do not depend on the batching
        const size_t npix = (size_t)rows * cols;
        const int batch = (int)std::max<size_t>(1, std::min<size_t>(n, ((size_t)512 << 20) / (npix * 9)));
        for (int i0 = 0; i0 < n; i0 += batch) {
            const int k = std::min(batch, n - i0);
            if (add_batch(tr, k, rows, cols, depth + i0 * npix, mask + i0 * npix, hipMemcpyHostToDevice)) return 1;
        }
        return 0;
    } catch (const std::exception& e) { avt_set_error(std::string("avt_rtree_trainer_add_images: ") + e.what()); return 1; }
    catch (...) { avt_set_error("avt_rtree_trainer_add_images: unknown exception"); return 1; }
}

int avt_rtree_trainer_info(const avt_rtree_trainer* tr, int* n_images, long long* n_samples) {
    if (!tr) { avt_set_error("avt_rtree_trainer_info: null trainer"); return 1; }
    if (n_images) *n_images = (int)tr->imgs.size();
    if (n_samples) *n_samples = tr->n_samples;
    return 0;
}

int avt_rtree_trainer_samples(avt_rtree_trainer* tr, int* image, int* x, int* y, unsigned char* label) {
    try {
        if (!tr) { avt_set_error("avt_rtree_trainer_samples: null trainer"); return 1; }
        const size_t n = (size_t)tr->n_samples;
        if (!n) return 0;
        TR_HIP(hipSetDevice(tr->device));
        std::vector<int> xy(n);
        if (image) TR_HIP(hipMemcpyAsync(image, tr->s.img.p, n * sizeof(int), hipMemcpyDeviceToHost, tr->stream));
        TR_HIP(hipMemcpyAsync(xy.data(), tr->s.xy.p, n * sizeof(int), hipMemcpyDeviceToHost, tr->stream));
        if (label) TR_HIP(hipMemcpyAsync(label, tr->s.lab.p, n, hipMemcpyDeviceToHost, tr->stream));
        TR_HIP(hipStreamSynchronize(tr->stream));
        for (size_t i = 0; i < n; ++i) {
            if (x) x[i] = xy[i] & 0xffff;
            if (y) y[i] = xy[i] >> 16;
        }
        return 0;
    } catch (const std::exception& e) { avt_set_error(std::string("avt_rtree_trainer_samples: ") + e.what()); return 1; }
    catch (...) { avt_set_error("avt_rtree_trainer_samples: unknown exception"); return 1; }
}

int avt_rtree_trainer_run(avt_rtree_trainer* tr, int part_map_len, const int* part_map, int part_map_type, avt_rtree** out, avt_rtree_train_stats* stats) {
    try {
        if (!tr || !out || part_map_len < 0 || (part_map_len > 0 && !part_map)) { avt_set_error("avt_rtree_trainer_run: bad arguments"); return 1; }
        if (tr->n_samples <= 0) { avt_set_error("avt_rtree_trainer_run: no samples (add images with labelled pixels first)"); return 1; }
        if (tr->n_samples >= (1ll << 31)) { avt_set_error("avt_rtree_trainer_run: more than 2^31 - 1 samples"); return 1; }
        TR_HIP(hipSetDevice(tr->device));
        return train(tr, part_map_len, part_map, part_map_type, out, stats);
    } catch (const std::exception& e) { avt_set_error(std::string("avt_rtree_trainer_run: ") + e.what()); return 1; }
    catch (...) { avt_set_error("avt_rtree_trainer_run: unknown exception"); return 1; }
}

int avt_rtree_transfer_images(avt_rtree* rt, int n, int rows, int cols, const float* depth, const unsigned char* mask, int* n_unvisited) {
    try {
        if (!rt || rt->device < 0 || !rt->d_nodes) { avt_set_error("avt_rtree_transfer_images: needs a tree on a device"); return 1; }
        avt_rtree_trainer probe;
        if (check_args(&probe, n, rows, cols, depth, mask, "avt_rtree_transfer_images")) return 1;
        if (transfer_add(rt, n, rows, cols, depth, mask, hipMemcpyHostToDevice, "avt_rtree_transfer_images")) return 1;
        return transfer_finish(rt, n_unvisited);
    } catch (const std::exception& e) { avt_set_error(std::string("avt_rtree_transfer_images: ") + e.what()); return 1; }
    catch (...) { avt_set_error("avt_rtree_transfer_images: unknown exception"); return 1; }
}

int avt_rtree_transfer_rendered(avt_rtree* rt, avt_renderer* r) {
    try {
        if (!rt || rt->device < 0 || !rt->d_nodes || !r) { avt_set_error("avt_rtree_transfer_rendered: needs a tree on a device and a renderer"); return 1; }
        TR_HIP(hipSetDevice(rt->device));
        const float* depth = nullptr;
        const unsigned char* mask = nullptr;
        int n = 0, w = 0, h = 0;
        if (avt_renderer_images_for(r, rt->stream, &depth, &mask, &n, &w, &h)) return 1;
        return transfer_add(rt, n, h, w, depth, mask, hipMemcpyDeviceToDevice, "avt_rtree_transfer_rendered");
    } catch (const std::exception& e) { avt_set_error(std::string("avt_rtree_transfer_rendered: ") + e.what()); return 1; }
    catch (...) { avt_set_error("avt_rtree_transfer_rendered: unknown exception"); return 1; }
}

int avt_rtree_transfer_finish(avt_rtree* rt, int* n_unvisited) {
    try {
        if (!rt || rt->device < 0 || !rt->d_nodes) { avt_set_error("avt_rtree_transfer_finish: needs a tree on a device"); return 1; }
        return transfer_finish(rt, n_unvisited);
    } catch (const std::exception& e) { avt_set_error(std::string("avt_rtree_transfer_finish: ") + e.what()); return 1; }
    catch (...) { avt_set_error("avt_rtree_transfer_finish: unknown exception"); return 1; }
}

int avt_rtree_trainer_add_rendered(avt_rtree_trainer* tr, avt_renderer* r) {
    try {
        if (!tr || !r) { avt_set_error("avt_rtree_trainer_add_rendered: null argument"); return 1; }
        TR_HIP(hipSetDevice(tr->device));
        const float* depth = nullptr;
        const unsigned char* mask = nullptr;
        int n = 0, w = 0, h = 0;
        if (avt_renderer_images_for(r, tr->stream, &depth, &mask, &n, &w, &h)) return 1;
        if (check_args(tr, n, h, w, depth, mask, "avt_rtree_trainer_add_rendered")) return 1;
        return add_batch(tr, n, h, w, depth, mask, hipMemcpyDeviceToDevice);
    } catch (const std::exception& e) { avt_set_error(std::string("avt_rtree_trainer_add_rendered: ") + e.what()); return 1; }
    catch (...) { avt_set_error("avt_rtree_trainer_add_rendered: unknown exception"); return 1; }
}

int avt_rtree_trainer_root_histograms(avt_rtree_trainer* tr, int n_features, int* hist, float* minmax) {
    try {
        if (!tr || n_features < 1 || !hist) { avt_set_error("avt_rtree_trainer_root_histograms: bad arguments"); return 1; }
        if (tr->n_samples <= 0) { avt_set_error("avt_rtree_trainer_root_histograms: no samples"); return 1; }
        TR_HIP(hipSetDevice(tr->device));
        return root_histograms(tr, n_features, hist, minmax);
    } catch (const std::exception& e) { avt_set_error(std::string("avt_rtree_trainer_root_histograms: ") + e.what()); return 1; }
    catch (...) { avt_set_error("avt_rtree_trainer_root_histograms: unknown exception"); return 1; }
}

}  // extern "C"
