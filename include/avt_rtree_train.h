/* avt_rtree_train.h — C ABI of the body-part forest TRAINER on the GPU, part of libavatar_hip.so.
 *
 * The reference trains its forests with AvatarTrainerV3 (RTree.cpp:2338-2950, behind RTree::trainFromAvatar,
 * :3292-3330) on CPU threads, and re-fits the leaves of a fixed tree with RTree::trainTransfer (:3332-3420).  This
 * header restates both on the device; include/ark/RTree.h re-creates the C++ calls on top.  The trained tree is an
 * avt_rtree (include/avt_rtree.h): ready for avt_rtree_predict_best and avt_rtree_export.
 *
 * What the trainer computes (reference file:line, the semantics DESIGN.md §8 lists):
 *   samples     every image contributes up to num_points_per_image pixels with part_mask != 255, chosen by a partial
 *               Fisher-Yates over the candidates in raster order (random_util::choose, include/Util.h:242-250); an image
 *               with no more candidates than that contributes all of them in raster order (initTraining, :2424-2497).
 *               A labelled pixel of depth 0 is a valid sample and scores 0.
 *   nodes       depth counts down from max_tree_depth; leaf if depth <= 1 or n <= min_samples; otherwise num_features
 *               random features, each scored with the threshold search of optimalInformationGain3 (:2782-2851) over
 *               T = min_samples_per_feature buckets; the best one splits the node stably (score < thresh: left), an empty
 *               side makes the node a leaf, a best gain of exactly 0 makes both children leaves (trainFromNode, :2501-2647).
 *   leaves      leaf[p] = (float)count_p / (float)n.
 *   numbering   the reference's depth-first order: children appended as a pair when their parent splits, left subtree
 *               before right, leaf ids in the order leaves are reached.
 *
 * Deliberate differences (the reference cannot be reproduced: it draws from a thread-local xorshift seeded by
 * std::random_device and settles ties by a thread race):
 *   randomness  a counter-based hash keyed by (seed, stable ids), spelled out below, so the tree does not depend on the
 *               order in which images or nodes are processed, nor on how images are split into add_* batches;
 *   ties        of bit-equal gains: the lower feature index wins;
 *   gains       in double, with the reference's formula and its sequential order over parts;
 *   counts      integers (the reference's float counts are exact only below 2^24);
 *   storage     each image is kept as the crop to its bounding box of non-zero depth (lossless: outside the image and
 *               zero depth both read BACKGROUND_DEPTH); a sample's own depth is read from the full image.
 * Parameters of the reference's trainers that do not change V3's result (num_threads, num_features_filtered,
 * frac_samples_per_feature, threshes_per_feature, max_images_loaded, mem_limit_mb, train_partial_save_path) have no
 * counterpart here.  num_parts x min_samples_per_feature is limited to 8192 (the bucket histogram lives in LDS: up to
 * 131 128 bytes per workgroup, asked of the device in avt_rtree_trainer_create, which refuses a parameter set whose
 * LDS the device cannot give; an accepted one never fails for it in avt_rtree_trainer_run).
 *
 * Functions return 0 on success; avt_last_error() (avt.h) describes a failure.
 */
#ifndef AVT_RTREE_TRAIN_H_
#define AVT_RTREE_TRAIN_H_

#include <stdint.h>

#include "avt_rtree.h"
#include "avt_render.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct avt_rtree_trainer avt_rtree_trainer;

/* RTree::trainFromAvatar's parameters that V3 reads (include/RTree.h:112-132). */
typedef struct avt_rtree_train_params {
    int num_parts;                /* numParts, 1..127; every label of a part mask must be < num_parts or 255      */
    int num_points_per_image;     /* samples per image (>= 1)                                                      */
    int num_features;             /* random features tried per internal node (>= 1)                                */
    float max_probe_offset;       /* feature components lie in [0.5, max_probe_offset) x {-1, +1, +3}; > 0.5       */
    int min_samples;              /* a node with n <= min_samples samples is a leaf (>= 0)                         */
    int max_tree_depth;           /* 1..AVT_RTREE_TRAIN_MAX_DEPTH; 1: the root is a leaf                           */
    int min_samples_per_feature;  /* T, the number of threshold buckets (the reference's misnomer), >= 1           */
    uint64_t seed;                /* keys every random draw below                                                  */
} avt_rtree_train_params;

#define AVT_RTREE_TRAIN_MAX_DEPTH 64

typedef struct avt_rtree_train_stats {
    int n_nodes, n_leafs, n_levels, n_images;
    long long n_samples;
    double total_ms;                                   /* avt_rtree_trainer_run, wall clock                          */
    int level_nodes[AVT_RTREE_TRAIN_MAX_DEPTH];        /* open nodes of level l (root: level 0)                      */
    int level_searched[AVT_RTREE_TRAIN_MAX_DEPTH];     /* ... of which searched for a split                          */
    long long level_evals[AVT_RTREE_TRAIN_MAX_DEPTH];  /* feature evaluations: sum over searched nodes of n x F      */
    double level_ms[AVT_RTREE_TRAIN_MAX_DEPTH];        /* wall clock of the level, host wait included                */
    int level_large[AVT_RTREE_TRAIN_MAX_DEPTH];        /* searched nodes of >= 2048 samples: one 256-thread workgroup */
                                                       /* per (node, chunk of features) instead of one wave          */
} avt_rtree_train_stats;

/* ---- the random draws, bit for bit (a restatement reproduces them from this text) ----------------------------------
 * splitmix64(x): z = x + 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) *
 *                0x94D049BB133111EB; return z ^ (z >> 31)                        (all uint64 arithmetic, wrapping)
 * hash(s, a, b) = splitmix64(splitmix64(splitmix64(s) ^ a) ^ b)
 * sample choice, image idx (counted across add_* calls from 0), step j, c candidates:
 *     r = j + hash(seed ^ AVT_RT_TAG_SAMPLE, idx, j) % (c - j)                    (randint(j, c - 1), inclusive)
 * feature f (0-based) of the node with path key k (root 1, children 2k + 0 left, 2k + 1 right), component
 * c = 0 u.x, 1 u.y, 2 v.x, 3 v.y, with h = hash(seed ^ AVT_RT_TAG_FEATURE, k, 4 f + c) and M = max_probe_offset:
 *     x = 0.5f + (M - 0.5f) * ((float)(h >> 40) * (1.0f / 16777216.0f))       (float, every operation rounded, no
 *                                                                                contraction)
 *     if (!(x < M)) x = the largest float below M                               (keeps [0.5, M) under rounding)
 *     component = x * (float)((int)((uint32_t)h % 3u) * 2 - 1)                  (factor -1, +1 or +3)
 * The factor +3 is the reference's: randint(0, 2) includes both ends (include/Util.h:224-238), so
 * randint(0, 2) * 2 - 1 is -1, +1 or +3 (RTree.cpp:2575-2578).  Kept: it is part of what the reference's forests are.
 * Path keys are 64-bit: they stay distinct up to AVT_RTREE_TRAIN_MAX_DEPTH levels. */
#define AVT_RT_TAG_SAMPLE 0x73616d706c657321ull
#define AVT_RT_TAG_FEATURE 0x6665617475726521ull

#if defined(__HIPCC__) || defined(__HIP__)
#define AVT_RT_HD __host__ __device__
#else
#define AVT_RT_HD
#endif

static inline AVT_RT_HD uint64_t avt_rt_splitmix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static inline AVT_RT_HD uint64_t avt_rt_hash(uint64_t s, uint64_t a, uint64_t b) {
    return avt_rt_splitmix64(avt_rt_splitmix64(avt_rt_splitmix64(s) ^ a) ^ b);
}
/* must be compiled without floating-point contraction (the library's copy is) */
static inline AVT_RT_HD float avt_rt_feature_component(uint64_t seed, uint64_t key, int f, int c, float max_probe_offset) {
    const uint64_t h = avt_rt_hash(seed ^ AVT_RT_TAG_FEATURE, key, (uint64_t)f * 4u + (uint64_t)c);
    const float u01 = (float)(h >> 40) * (1.0f / 16777216.0f);
    const float span = max_probe_offset - 0.5f;
    const float scaled = span * u01;
    float x = 0.5f + scaled;
    if (!(x < max_probe_offset)) {
        union { float f; uint32_t u; } b;
        b.f = max_probe_offset;
        b.u -= 1u;
        x = b.f;
    }
    return x * (float)((int)((uint32_t)h % 3u) * 2 - 1);
}

/* trainFromAvatar's xorKey (RTree.cpp:447: a random uint32 in [1, 2^32 - 1]) derived from the seed: the high half of
 * hash(seed, AVT_RT_TAG_XOR, 0), 1 if that is 0.  Image idx is the avatar posed by randomize(true, true, true, idx ^ xorKey). */
#define AVT_RT_TAG_XOR 0x786f726b65792121ull
static inline uint32_t avt_rt_xor_key(uint64_t seed) {
    const uint32_t k = (uint32_t)(avt_rt_hash(seed, AVT_RT_TAG_XOR, 0) >> 32);
    return k ? k : 1u;
}

/* Creates an empty trainer on `device` with the given parameters (copied). */
int avt_rtree_trainer_create(int device, const avt_rtree_train_params* params, avt_rtree_trainer** out);
void avt_rtree_trainer_destroy(avt_rtree_trainer* tr);

/* Adds n host images (row-major, n x rows x cols each): depth float32 metres (0 = background, finite, >= 0) and part
 * masks uint8 (255 = none, else < num_parts).  Samples are chosen on the device; images get the next indices. */
int avt_rtree_trainer_add_images(avt_rtree_trainer* tr, int n, int rows, int cols, const float* depth, const unsigned char* part_mask);

/* Adds the depth and part-mask images of r's last avt_renderer_run (it must have rendered AVT_RENDER_DEPTH |
 * AVT_RENDER_PART_MASK; all resident avatars, in order), copied device to device after the work queued on the renderer -
 * the way avt_renderer_from_ctx orders its copies - on the same device.  Same rules and checks as add_images; returns once
 * the renderer's buffers are no longer read. */
int avt_rtree_trainer_add_rendered(avt_rtree_trainer* tr, avt_renderer* r);

/* n_images added so far and the number of samples chosen from them. */
int avt_rtree_trainer_info(const avt_rtree_trainer* tr, int* n_images, long long* n_samples);
/* Copies the samples out in the trainer's order (image-major; within an image in the order they were chosen).  Any
 * pointer may be NULL; each array holds n_samples entries. */
int avt_rtree_trainer_samples(avt_rtree_trainer* tr, int* image, int* x, int* y, unsigned char* label);

/* Test hook: the root's integer (num_parts x T) bucket histograms of features 0 .. n_features - 1 as the search kernel counts
 * them (hist: n_features x num_parts x T, row-major) and the scores' min / max per feature (minmax: n_features x 2). */
int avt_rtree_trainer_root_histograms(avt_rtree_trainer* tr, int n_features, int* hist, float* minmax);

/* Trains one tree from every sample added so far (refused when there are none) and returns it as a new avt_rtree on
 * the trainer's device carrying the given part map (part_map_len 0: none).  `stats` may be NULL.  May be called
 * again: the samples are kept. */
int avt_rtree_trainer_run(avt_rtree_trainer* tr, int part_map_len, const int* part_map, int part_map_type, avt_rtree** out,
                          avt_rtree_train_stats* stats);

/* RTree::trainTransfer (RTree.cpp:3332-3420) over n host images: every pixel with part_mask != 255 walks the fixed tree
 * (probes bounded by the image); integer counts per (leaf, part); a leaf with a count gets count / sum, a leaf never
 * reached keeps its weights and is counted in *n_unvisited (may be NULL); then leafBestMatch is rebuilt. */
int avt_rtree_transfer_images(avt_rtree* rt, int n, int rows, int cols, const float* depth, const unsigned char* part_mask, int* n_unvisited);
/* The same over many batches on the device: avt_rtree_transfer_rendered adds the counts of r's last depth + part-mask run
 * (copied device to device after the renderer's queued work; a label >= num_parts is refused and the batch's counts are
 * dropped), avt_rtree_transfer_finish turns every count added so far into the leaf distributions as above and starts over. */
int avt_rtree_transfer_rendered(avt_rtree* rt, avt_renderer* r);
int avt_rtree_transfer_finish(avt_rtree* rt, int* n_unvisited);

#ifdef __cplusplus
}
#endif
#endif
