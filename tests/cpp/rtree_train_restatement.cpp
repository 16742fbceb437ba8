// rtree_train_restatement.cpp — CPU restatement of the reference's forest trainer (AvatarTrainerV3, RTree.cpp:2338-2950) and of
// RTree::trainTransfer (:3332-3420) with the port's documented differences (include/avt_rtree_train.h: the hash draws, ties to
// the lower feature index, gains in double, integer counts), for the tests of the GPU trainer.  Compiled at test time with
// g++ -O2 -ffp-contract=off -pthread.  TEST INFRASTRUCTURE ONLY.
//
// Near ties: where the device's log2 may round one ulp away from glibc's, two gains within 1e-12 relative - of two features at a
// node, or of two thresholds of one feature - take the device's choice when its tree is given; they are counted.
//
// Unlike the device, which trains level by level, this keeps the reference's RECURSIVE depth-first structure
// (trainFromNode), so comparing the two trees checks the device's renumbering against the reference's order.  With
// nthreads > 1 the features of a node are scored on that many threads (it then doubles as the CPU baseline).
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <thread>
#include <vector>

namespace {

// the draws, restated from the text of include/avt_rtree_train.h
const uint64_t kTagSample = 0x73616d706c657321ull, kTagFeature = 0x6665617475726521ull;
uint64_t sm64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
uint64_t hash3(uint64_t s, uint64_t a, uint64_t b) { return sm64(sm64(sm64(s) ^ a) ^ b); }
float component(uint64_t seed, uint64_t key, int f, int c, float M) {
    const uint64_t h = hash3(seed ^ kTagFeature, key, (uint64_t)f * 4 + c);
    const float u01 = (float)(h >> 40) * (1.0f / 16777216.0f);
    float x = 0.5f + (M - 0.5f) * u01;
    if (!(x < M)) x = std::nextafter(M, 0.f);
    const int k = (int)((uint32_t)h % 3u);      // randint(0, 2): -1, +1, +3
    return x * (float)(k * 2 - 1);
}

struct Img { int rows, cols; const float* d; const unsigned char* m; };
struct Sample { int img, x, y, label; float depth; };
struct Feat { float u[2], v[2]; };

float get_depth(const Img& im, int x, int y) {                 // getDepth, RTree.cpp:41-50 (image bounds)
    if (y < 0 || x < 0 || y >= im.rows || x >= im.cols) return 20.f;
    const float z = im.d[(size_t)y * im.cols + x];
    return z == 0.0f ? 20.f : z;
}
float score(const Img& im, const Sample& s, const Feat& f) {   // scoreByFeature, :52-68
    if (s.depth == 0.f) return 0.f;                            // u / 0: every probe leaves the image (x86 int cast)
    const int ux = (int32_t)std::round(f.u[0] / s.depth) + s.x, uy = (int32_t)std::round(f.u[1] / s.depth) + s.y;
    const int vx = (int32_t)std::round(f.v[0] / s.depth) + s.x, vy = (int32_t)std::round(f.v[1] / s.depth) + s.y;
    return get_depth(im, ux, uy) - get_depth(im, vx, vy);
}

// the threshold scan of optimalInformationGain3 (:2821-2848) over a (parts x T) bucket histogram and the node totals;
// returns the best bucket index (-1: no threshold with two non-empty sides) and its gain
int scan(int P, int T, const std::vector<long long>& hist, const std::vector<long long>& tot, double* gain, std::vector<double>* all = nullptr) {
    std::vector<long long> left(tot), right(P, 0);
    double best = -std::numeric_limits<double>::infinity();
    int bi = -1;
    for (int i = 0; i < T; ++i) {
        for (int p = 0; p < P; ++p) { left[p] -= hist[(size_t)p * T + i]; right[p] += hist[(size_t)p * T + i]; }
        long long ls = 0, rs = 0;
        for (int p = 0; p < P; ++p) { ls += left[p]; rs += right[p]; }
        if (all) all->push_back(std::numeric_limits<double>::quiet_NaN());
        if (ls == 0 || rs == 0) continue;                      // the reference's NaN: never chosen
        double hl = 0.0, hr = 0.0;
        for (int p = 0; p < P; ++p) {                          // entropy, :28-39, in double
            const double pl = (double)left[p] / (double)ls;
            if (!(pl < 1e-10)) hl -= pl * std::log2(pl);
        }
        for (int p = 0; p < P; ++p) {
            const double pr = (double)right[p] / (double)rs;
            if (!(pr < 1e-10)) hr -= pr * std::log2(pr);
        }
        const double g = -((double)ls * hl + (double)rs * hr);
        if (all) all->back() = g;
        if (g > best) { best = g; bi = i; }
    }
    *gain = best;
    return bi;
}

size_t bucket_of(float sc, float mn, float step) { return static_cast<size_t>((sc - mn) / step); }

struct Trainer {
    int P, K, F, min_samples, max_depth, T;
    float M;
    uint64_t seed;
    int nthreads;
    std::vector<Img> imgs;
    std::vector<Sample> samples;
    // output
    std::vector<float> feature;   // n x 5
    std::vector<int> links;       // n x 3
    std::vector<float> leaf;      // nl x P
    // device tree (optional): near ties take its choice
    int dev_n = 0;
    const float* dev_feature = nullptr;
    const int* dev_links = nullptr;
    int ties = 0;
    // nodes at which two gains that are not bit-equal lie within 1e-12 relative - the best feature's and another feature's, or the
    // best and another threshold of the chosen feature - counted from this restatement alone: `ties` can never exceed it
    int near = 0;

    void choose_samples() {
        for (int i = 0; i < (int)imgs.size(); ++i) {
            const Img& im = imgs[i];
            std::vector<int> cand;
            for (int r = 0; r < im.rows; ++r)
                for (int c = 0; c < im.cols; ++c)
                    if (im.m[(size_t)r * im.cols + c] != 255) cand.push_back(r * im.cols + c);
            std::vector<int> chosen;
            if ((int)cand.size() > K) {                        // random_util::choose, Util.h:242-250
                for (int j = 0; j < K; ++j) {
                    const int r = j + (int)(hash3(seed ^ kTagSample, (uint64_t)i, (uint64_t)j) % (uint64_t)(cand.size() - j));
                    chosen.push_back(cand[r]);
                    std::swap(cand[j], cand[r]);
                }
            } else {
                chosen = cand;
            }
            for (int p : chosen) samples.push_back(Sample{i, p % im.cols, p / im.cols, im.m[p], im.d[p]});
        }
    }

    Feat feat(uint64_t key, int f) const {
        return Feat{{component(seed, key, f, 0, M), component(seed, key, f, 1, M)}, {component(seed, key, f, 2, M), component(seed, key, f, 3, M)}};
    }

    // optimalInformationGain3 for one feature: gain (-inf if no valid threshold) and threshold
    double info_gain(size_t start, size_t end, const Feat& f, float* thresh, std::vector<double>* all = nullptr, std::vector<float>* all_t = nullptr) const {
        float mn = std::numeric_limits<float>::max(), mx = std::numeric_limits<float>::lowest();
        std::vector<long long> tot(P, 0), hist((size_t)P * T, 0);
        std::vector<float> sc(end - start);
        for (size_t i = start; i < end; ++i) {
            sc[i - start] = score(imgs[samples[i].img], samples[i], f);
            mn = std::min(sc[i - start], mn);
            mx = std::max(sc[i - start], mx);
            tot[samples[i].label] += 1;
        }
        const float step = (mx - mn + std::numeric_limits<float>::epsilon()) / (T + 1.f);
        for (size_t i = start; i < end; ++i) {
            const size_t b = bucket_of(sc[i - start], mn, step);
            if (b < (size_t)T) hist[(size_t)samples[i].label * T + b] += 1;
        }
        double g;
        const int bi = scan(P, T, hist, tot, &g, all);
        if (all_t)
            for (int i = 0; i < T; ++i) all_t->push_back(mn + (i + 1) * step);
        if (bi < 0) return -std::numeric_limits<double>::infinity();
        *thresh = mn + (bi + 1) * step;
        return g;
    }

    void make_leaf(int id, size_t start, size_t end) {
        links[3 * (size_t)id + 2] = (int)(leaf.size() / P);
        std::vector<long long> cnt(P, 0);
        for (size_t i = start; i < end; ++i) cnt[samples[i].label] += 1;
        for (int p = 0; p < P; ++p) leaf.push_back((float)cnt[p] / (float)(end - start));
    }

    int new_node() {
        feature.insert(feature.end(), 5, 0.f);
        links.insert(links.end(), {-1, -1, -1});
        return (int)(links.size() / 3) - 1;
    }

    // trainFromNode, :2501-2647
    void node(int id, uint64_t key, size_t start, size_t end, int depth) {
        if (depth <= 1 || end - start <= (size_t)min_samples) { make_leaf(id, start, end); return; }
        std::vector<double> gains(F);
        std::vector<float> ths(F, 0.f);
        auto work = [&](int t) {
            for (int f = t; f < F; f += nthreads) gains[f] = info_gain(start, end, feat(key, f), &ths[f]);
        };
        if (nthreads <= 1) work(0);
        else {
            std::vector<std::thread> th;
            for (int t = 0; t < nthreads; ++t) th.emplace_back(work, t);
            for (auto& x : th) x.join();
        }
        int bf = -1;
        double bg = -std::numeric_limits<double>::infinity(), g2 = bg;
        for (int f = 0; f < F; ++f) {
            if (gains[f] > bg) { g2 = bg; bg = gains[f]; bf = f; }
            else if (gains[f] > g2) g2 = gains[f];
        }
        if (bf < 0) { make_leaf(id, start, end); return; }       // no feature with a valid threshold: the split would be empty
        {
            auto close = [&](double g) { return g != bg && std::fabs(bg - g) <= 1e-12 * std::fabs(bg); };
            bool nt = false;
            for (int f = 0; f < F && !nt; ++f) nt = f != bf && close(gains[f]);
            if (!nt) {
                std::vector<double> all;
                float t0;
                info_gain(start, end, feat(key, bf), &t0, &all);
                for (double g : all) nt = nt || close(g);          // NaN (an empty side) compares false
            }
            near += nt;
        }
        if (dev_feature && id < dev_n && dev_links[3 * (size_t)id + 2] < 0 && std::isfinite(g2) && std::fabs(bg - g2) <= 1e-12 * std::fabs(bg)) {
            // near tie: the device's log2 may be one ulp away from glibc's; take the device's choice among the tied features
            for (int f = 0; f < F; ++f) {
                if (!(std::fabs(bg - gains[f]) <= 1e-12 * std::fabs(bg))) continue;
                const Feat ft = feat(key, f);
                const float* df = dev_feature + 5 * (size_t)id;
                if (ft.u[0] == df[0] && ft.u[1] == df[1] && ft.v[0] == df[2] && ft.v[1] == df[3]) {
                    if (f != bf) ++ties;
                    bf = f; bg = gains[f];
                    break;
                }
            }
        }
        const Feat best = feat(key, bf);
        float th = ths[bf];
        if (dev_feature && id < dev_n && dev_links[3 * (size_t)id + 2] < 0) {
            // near tie between two thresholds of the chosen feature (the same log2 ulp): take the device's threshold
            const float* df = dev_feature + 5 * (size_t)id;
            if (best.u[0] == df[0] && best.u[1] == df[1] && best.v[0] == df[2] && best.v[1] == df[3] && df[4] != th) {
                std::vector<double> all;
                std::vector<float> all_t;
                float t0;
                info_gain(start, end, best, &t0, &all, &all_t);
                for (int i = 0; i < T; ++i)
                    if (all_t[i] == df[4] && std::fabs(all[i] - bg) <= 1e-12 * std::fabs(bg)) { th = df[4]; bg = all[i]; ++ties; break; }
            }
        }
        // split, :2853-2928: stable, score < thresh to the left
        const size_t mid = std::stable_partition(samples.begin() + start, samples.begin() + end,
                                                 [&](const Sample& s) { return score(imgs[s.img], s, best) < th; }) - samples.begin();
        if (mid == start || mid == end) { make_leaf(id, start, end); return; }
        float* fo = &feature[5 * (size_t)id];
        fo[0] = best.u[0]; fo[1] = best.u[1]; fo[2] = best.v[0]; fo[3] = best.v[1]; fo[4] = th;
        const int l = new_node(), r = new_node();
        links[3 * (size_t)id] = l;
        links[3 * (size_t)id + 1] = r;
        if (bg == 0.0) {
            node(l, 2 * key, start, mid, 0);
            node(r, 2 * key + 1, mid, end, 0);
        } else {
            node(l, 2 * key, start, mid, depth - 1);
            node(r, 2 * key + 1, mid, end, depth - 1);
        }
    }
};

struct Result {
    std::vector<Sample> samples;
    std::vector<float> feature, leaf;
    std::vector<int> links;
    int ties = 0, near = 0;
};

}  // namespace

extern "C" {

void* rst_train(int n, int rows, int cols, const float* depth, const unsigned char* mask, int num_parts, int k, int F, float max_probe, int min_samples,
                int max_depth, int T, uint64_t seed, int nthreads, int dev_n, const float* dev_feature, const int* dev_links, int train) {
    Trainer t{num_parts, k, F, min_samples, max_depth, T, max_probe, seed, std::max(1, nthreads)};
    for (int i = 0; i < n; ++i) t.imgs.push_back(Img{rows, cols, depth + (size_t)i * rows * cols, mask + (size_t)i * rows * cols});
    t.dev_n = dev_n; t.dev_feature = dev_feature; t.dev_links = dev_links;
    t.choose_samples();
    Result* r = new Result();
    r->samples = t.samples;
    if (train && !t.samples.empty()) {
        t.new_node();
        t.node(0, 1, 0, t.samples.size(), max_depth);
    }
    r->feature = t.feature; r->links = t.links; r->leaf = t.leaf; r->ties = t.ties; r->near = t.near;
    return r;
}

void rst_sizes(void* h, long long* n_samples, int* n_nodes, int* n_leafs, int* ties) {
    Result* r = (Result*)h;
    *n_samples = (long long)r->samples.size();
    *n_nodes = (int)(r->links.size() / 3);
    int nl = 0;
    for (size_t i = 0; i < r->links.size() / 3; ++i) nl += r->links[3 * i + 2] >= 0;
    *n_leafs = nl;
    *ties = r->ties;
}

void rst_get(void* h, int* img, int* x, int* y, unsigned char* label, float* feature, int* links, float* leaf) {
    Result* r = (Result*)h;
    for (size_t i = 0; i < r->samples.size(); ++i) {
        img[i] = r->samples[i].img; x[i] = r->samples[i].x; y[i] = r->samples[i].y; label[i] = (unsigned char)r->samples[i].label;
    }
    std::copy(r->feature.begin(), r->feature.end(), feature);
    std::copy(r->links.begin(), r->links.end(), links);
    std::copy(r->leaf.begin(), r->leaf.end(), leaf);
}

int rst_near(void* h) { return ((Result*)h)->near; }

void rst_free(void* h) { delete (Result*)h; }

// trainTransfer (:3332-3420) over a fixed tree: leaf (nl x P) is updated in place; returns the number of unvisited leaves
int rst_transfer(int n_nodes, const float* feature, const int* links, int nl, int P, float* leaf, int n, int rows, int cols, const float* depth,
                 const unsigned char* mask) {
    std::vector<unsigned long long> cnt((size_t)nl * P, 0);
    for (int i = 0; i < n; ++i) {
        const Img im{rows, cols, depth + (size_t)i * rows * cols, mask + (size_t)i * rows * cols};
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < cols; ++c) {
                const int lab = im.m[(size_t)r * cols + c];
                if (lab == 255) continue;
                const Sample s{i, c, r, lab, im.d[(size_t)r * cols + c]};
                int id = 0;
                while (links[3 * id + 2] == -1) {
                    const float* f = feature + 5 * (size_t)id;
                    id = score(im, s, Feat{{f[0], f[1]}, {f[2], f[3]}}) < f[4] ? links[3 * id] : links[3 * id + 1];
                }
                cnt[(size_t)links[3 * id + 2] * P + lab] += 1;
            }
    }
    int zero = 0;
    for (int l = 0; l < nl; ++l) {
        unsigned long long sum = 0;
        for (int p = 0; p < P; ++p) sum += cnt[(size_t)l * P + p];
        if (sum > 0)
            for (int p = 0; p < P; ++p) leaf[(size_t)l * P + p] = (float)cnt[(size_t)l * P + p] / (float)sum;
        else
            ++zero;
    }
    (void)n_nodes;
    return zero;
}

// the root's bucket histograms (P x T, integer) and min / max of features 0 .. nf-1, as optimalInformationGain3 counts them
void rst_root_hist(int n, int rows, int cols, const float* depth, const unsigned char* mask, int num_parts, int k, float max_probe, int T, uint64_t seed,
                   int nf, int* hist, float* minmax) {
    Trainer t{num_parts, k, nf, 1, 2, T, max_probe, seed, 1};
    for (int i = 0; i < n; ++i) t.imgs.push_back(Img{rows, cols, depth + (size_t)i * rows * cols, mask + (size_t)i * rows * cols});
    t.choose_samples();
    for (int f = 0; f < nf; ++f) {
        const Feat ft = t.feat(1, f);
        float mn = std::numeric_limits<float>::max(), mx = std::numeric_limits<float>::lowest();
        std::vector<float> sc(t.samples.size());
        for (size_t i = 0; i < t.samples.size(); ++i) {
            sc[i] = score(t.imgs[t.samples[i].img], t.samples[i], ft);
            mn = std::min(sc[i], mn);
            mx = std::max(sc[i], mx);
        }
        const float step = (mx - mn + std::numeric_limits<float>::epsilon()) / (T + 1.f);
        int* h = hist + (size_t)f * num_parts * T;
        std::fill(h, h + (size_t)num_parts * T, 0);
        for (size_t i = 0; i < t.samples.size(); ++i) {
            const size_t b = bucket_of(sc[i], mn, step);
            if (b < (size_t)T) h[(size_t)t.samples[i].label * T + b] += 1;
        }
        minmax[2 * f] = mn;
        minmax[2 * f + 1] = mx;
    }
}

// known-answer hooks for tests/test_rtree_train_cpu.py
float rst_component(uint64_t seed, uint64_t key, int f, int c, float M) { return component(seed, key, f, c, M); }
uint64_t rst_hash(uint64_t s, uint64_t a, uint64_t b) { return hash3(s, a, b); }
long long rst_bucket(float score_, float mn, float mx, int T) {
    const float step = (mx - mn + std::numeric_limits<float>::epsilon()) / (T + 1.f);
    return (long long)bucket_of(score_, mn, step);
}
int rst_scan(int P, int T, const long long* hist, const long long* tot, double* gain) {
    return scan(P, T, std::vector<long long>(hist, hist + (size_t)P * T), std::vector<long long>(tot, tot + P), gain);
}

}  // extern "C"
