// ark/RTree.h — the reference's `ark::RTree` (include/RTree.h:12-184) re-created over the C ABI of avt_rtree.h:
// same class name, member names, defaults and call protocol for the inference side (loadFile, exportFile, predictBest,
// postProcess, numParts, partMap, leafData, leafBestMatch).  Inference, the batch forms and postProcess on the device are
// LabelHandle's (ark/LabelHandle.h, which also has the image and point types), shared with ark::RForest.
// Training runs on the GPU (include/avt_rtree_train.h): trainFromAvatar is the V3 trainer (RTree.cpp:2338-2950) on avatars
// skinned, rendered and sampled on the device; train(images...) feeds it in-memory depth images and part masks;
// trainTransfer(images...) re-fits the leaves (:3332-3420).  The V2 trainer of train(depth_dir, part_mask_dir, ...) is not built.
#pragma once
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../avt.h"
#include "../avt_rtree.h"
#include "../avt_rtree_train.h"
#include "Avatar.h"
#include "LabelHandle.h"
#include "Types.h"

namespace ark {

/** The C handle's type, the class name of the FATAL lines and the entry points of a tree, for LabelHandle */
struct RTreeApi {
    typedef avt_rtree Handle;
    static constexpr const char* name = "RTree";
    static constexpr auto predict_best = avt_rtree_predict_best;
    static constexpr auto predict = avt_rtree_predict;
    static constexpr auto images_upload = avt_rtree_images_upload;
    static constexpr auto predict_best_resident_boxes = avt_rtree_predict_best_resident_boxes;
    static constexpr auto predict_best_from_bgsub = avt_rtree_predict_best_from_bgsub;
    static constexpr auto labels_download_all = avt_rtree_labels_download_all;
    static constexpr auto labels_upload = avt_rtree_labels_upload;
    static constexpr auto post_process_resident = avt_rtree_post_process_resident;
    static constexpr auto post_process_from_bgsub = avt_rtree_post_process_from_bgsub;
    static constexpr auto com_pre_get = avt_rtree_com_pre_get;
    static constexpr auto com_pre_set = avt_rtree_com_pre_set;
};

class RTree : public LabelHandle<RTree, RTreeApi> {
    friend class LabelHandle<RTree, RTreeApi>;      // ensure()

public:
    typedef std::vector<float> Distribution;
    /** Assumed depth of background (meters), RTree.cpp:325 */
    static constexpr float BACKGROUND_DEPTH = 20.f;

    struct RNode {  // RTree.h:28-41
        float u[2] = {0, 0}, v[2] = {0, 0};
        float thresh = 0;
        int lnode = -1, rnode = -1;
        int leafid = -1;
    };

    /** Create empty RTree with number of different parts */
    explicit RTree(int num_parts, int device = 0) : numParts(num_parts), device_(device) {}
    /** Load data from path */
    explicit RTree(const std::string& path, int device = 0) : device_(device) {
        if (!loadFile(path)) fprintf(stderr, "ERROR: RTree failed to initialize from %s\n", path.c_str());
    }
    ~RTree() { avt_rtree_destroy(h_); }
    RTree(const RTree&) = delete;
    RTree& operator=(const RTree&) = delete;

    bool loadFile(const std::string& path) {
        avt_rtree_destroy(h_);
        h_ = nullptr;
        if (avt_rtree_load(path.c_str(), device_, &h_) != 0) return false;
        pull();
        return true;
    }
    bool exportFile(const std::string& path) { return ensure() && avt_rtree_export(h_, path.c_str()) == 0; }

    /** The V3 trainer (RTree.cpp:2338-2950) on in-memory images, parameters in the reference's order (include/RTree.h:88-105;
     *  defaults: rtree-train's command line).  num_threads and verbose are accepted and ignored.  Replaces this tree (numParts
     *  must be set); like the rest of this class a failure is fatal (message + exit). */
    void train(const std::vector<ImageF>& depth, const std::vector<Image8>& part_mask, int /*num_threads*/ = 0, bool /*verbose*/ = false,
               int num_points_per_image = 2000, int num_features = 5000, int max_probe_offset = 170, int min_samples = 1, int max_tree_depth = 20,
               int min_samples_per_feature = 20, uint64_t seed = 0, const std::vector<int>& part_map = {}, int part_map_type = 0) {
        if (depth.empty() || depth.size() != part_mask.size()) fatal("train", "need as many part masks as depth images, at least one");
        avt_rtree_trainer* tr = trainer(num_points_per_image, num_features, max_probe_offset, min_samples, max_tree_depth, min_samples_per_feature, seed);
        std::vector<float> d;
        std::vector<uint8_t> m;
        for (size_t i = 0; i < depth.size();) {          // runs of same-size images go in one call
            size_t j = i;
            d.clear(); m.clear();
            for (; j < depth.size() && depth[j].rows == depth[i].rows && depth[j].cols == depth[i].cols; ++j) {
                if (part_mask[j].rows != depth[j].rows || part_mask[j].cols != depth[j].cols) fatal("train", "a part mask differs in size from its depth image");
                d.insert(d.end(), depth[j].a.begin(), depth[j].a.end());
                m.insert(m.end(), part_mask[j].a.begin(), part_mask[j].a.end());
            }
            if (avt_rtree_trainer_add_images(tr, (int)(j - i), depth[i].rows, depth[i].cols, d.data(), m.data()) != 0) die("train");
            i = j;
        }
        finish_training(tr, part_map, part_map_type);
    }

    /** RTree::trainFromAvatar (include/RTree.h:112-132; the empty pose-sequence branch of AvatarDataSource, RTree.cpp:421-549):
     *  image idx is avatar_model posed by Avatar::randomize(true, true, true, idx ^ xorKey) (xorKey = avt_rt_xor_key(seed)),
     *  skinned by avt_lbs_update into a context of this call and rendered by the GPU renderer (renderDepth, renderPartMask with
     *  part_map), `batch` images at a time, handed to the trainer device to device.  numParts must be set; an empty part_map
     *  is the joint id itself.  The parameters V3 does not read are accepted and ignored. */
    void trainFromAvatar(AvatarModel& avatar_model, const CameraIntrin& intrin, const Size& image_size, int /*num_threads*/ = 0, bool /*verbose*/ = false,
                         int num_images = 30000, int num_points_per_image = 5000, int num_features = 2000, int /*num_features_filtered*/ = 200,
                         int max_probe_offset = 225, int min_samples = 100, int max_tree_depth = 20, int min_samples_per_feature = 20,
                         float /*frac_samples_per_feature*/ = 0.01f, int /*threshes_per_feature*/ = 15, const std::vector<int>& part_map = {},
                         int /*max_images_loaded*/ = 50, int /*mem_limit_mb*/ = 12000, const std::string& /*train_partial_save_path*/ = "",
                         uint64_t seed = 0, int batch = 64) {
        const int J = avatar_model.numJoints(), K = avatar_model.numShapeKeys();
        std::vector<int> pm(part_map);
        if (pm.empty()) for (int j = 0; j < J; ++j) pm.push_back(j);
        if ((int)pm.size() < J || num_images < 1 || batch < 1) fatal("trainFromAvatar", "part_map needs one entry per joint; num_images, batch >= 1");
        int np = 0;
        for (int v : pm) np = v + 1 > np ? v + 1 : np;
        avt_rtree_trainer* tr = trainer(num_points_per_image, num_features, max_probe_offset, min_samples, max_tree_depth, min_samples_per_feature, seed);
        avt_ctx* ctx = nullptr;
        avt_renderer* rend = nullptr;
        if (avt_ctx_create(device_, avatar_model.handle, np, pm.data(), 64, batch, &ctx) != 0 ||
            avt_renderer_create(device_, avatar_model.handle, image_size.width, image_size.height, intrin.fx, intrin.fy, intrin.cx, intrin.cy, batch,
                                &rend) != 0 ||
            avt_renderer_set_part_map(rend, (int)pm.size(), pm.data()) != 0)
            die("trainFromAvatar");
        const uint32_t xorKey = avt_rt_xor_key(seed);
        Avatar ava(avatar_model);
        std::vector<double> w, p, R;
        for (int i0 = 0; i0 < num_images; i0 += batch) {
            const int k = num_images - i0 < batch ? num_images - i0 : batch;
            w.assign((size_t)K * k, 0.0); p.assign((size_t)3 * k, 0.0); R.assign((size_t)9 * J * k, 0.0);
            for (int i = 0; i < k; ++i) {
                ava.randomize(true, true, true, (uint32_t)(i0 + i) ^ xorKey);
                for (int c = 0; c < K; ++c) w[(size_t)i * K + c] = ava.w[c];
                for (int c = 0; c < 3; ++c) p[(size_t)i * 3 + c] = ava.p(c);
                for (int j = 0; j < J; ++j)
                    for (int c = 0; c < 9; ++c) R[((size_t)i * J + j) * 9 + c] = ava.r[j].data()[c];
            }
            if (avt_lbs_update(ctx, k, w.data(), p.data(), R.data(), nullptr, nullptr, nullptr) != 0 || avt_renderer_from_ctx(rend, ctx, k, nullptr) != 0 ||
                avt_renderer_run(rend, AVT_RENDER_DEPTH | AVT_RENDER_PART_MASK) != 0 || avt_rtree_trainer_add_rendered(tr, rend) != 0)
                die("trainFromAvatar");
        }
        avt_renderer_destroy(rend);
        avt_ctx_destroy(ctx);
        finish_training(tr, pm, 0);
    }

    /** RTree::trainTransfer (RTree.cpp:3332-3420) over in-memory images of one size: returns the number of leaves never reached
     *  (they keep their weights); a failure is fatal. */
    int trainTransfer(const std::vector<ImageF>& depth, const std::vector<Image8>& part_mask, int /*num_threads*/ = 0, bool /*verbose*/ = false) {
        if (!ensure()) fatal("trainTransfer", "no tree");
        if (depth.empty() || depth.size() != part_mask.size()) fatal("trainTransfer", "need as many part masks as depth images, at least one");
        const int rows = depth[0].rows, cols = depth[0].cols;
        std::vector<float> d;
        std::vector<uint8_t> m;
        for (size_t i = 0; i < depth.size(); ++i) {
            if (depth[i].rows != rows || depth[i].cols != cols || part_mask[i].rows != rows || part_mask[i].cols != cols)
                fatal("trainTransfer", "the images must share one size");
            d.insert(d.end(), depth[i].a.begin(), depth[i].a.end());
            m.insert(m.end(), part_mask[i].a.begin(), part_mask[i].a.end());
        }
        int unvisited = 0;
        if (avt_rtree_transfer_images(h_, (int)depth.size(), rows, cols, d.data(), m.data(), &unvisited) != 0) die("trainTransfer");
        pull();
        return unvisited;
    }

    /** RTree.h:150-166 */
    void postProcess(Image8& image, MatrixNX<2>& com_pre, int interval = 1, int /*num_threads*/ = 1, Point top_left = Point(0, 0),
                     Point bot_right = Point(-1, -1), double dist_to_pre_weight = 0.001) {
        const bool valid = (int)com_pre.cols() == numParts;
        if (!valid) com_pre.resize(2, numParts);
        if (!ensure() || avt_rtree_post_process(h_, image.data(), image.rows, image.cols, com_pre.data(), valid ? 1 : 0, interval, top_left.x, top_left.y,
                                                bot_right.x, bot_right.y, dist_to_pre_weight) != 0)
            die("postProcess");
    }

    /** The C handle (ark::RForest copies the tree through it); a tree filled in through the public members is uploaded first.
     *  Null when the tree is empty. */
    avt_rtree* handle() { return ensure() ? h_ : nullptr; }

    std::vector<RNode> nodes;
    std::vector<Distribution> leafData;
    std::vector<uint8_t> leafBestMatch;
    int numParts = 0;
    std::vector<int> partMap;
    int partMapType = 0;

private:
    // a tree filled in through the public members (nodes / leafData) is uploaded on first use
    bool ensure() {
        if (h_) return true;
        if (nodes.empty()) return false;
        std::vector<float> f(5 * nodes.size()), ld;
        std::vector<int> l(3 * nodes.size());
        for (size_t i = 0; i < nodes.size(); ++i) {
            const RNode& n = nodes[i];
            f[5 * i] = n.u[0]; f[5 * i + 1] = n.u[1]; f[5 * i + 2] = n.v[0]; f[5 * i + 3] = n.v[1]; f[5 * i + 4] = n.thresh;
            l[3 * i] = n.lnode; l[3 * i + 1] = n.rnode; l[3 * i + 2] = n.leafid;
        }
        for (const Distribution& d : leafData) ld.insert(ld.end(), d.begin(), d.end());
        avt_rtree_desc d{(int)nodes.size(), (int)leafData.size(), numParts, f.data(), l.data(), ld.data(), (int)partMap.size(), partMap.data(), partMapType};
        if (avt_rtree_create(&d, device_, &h_) != 0) return false;
        pull();
        return true;
    }
    void pull() {
        int n = 0, nl = 0, pml = 0;
        avt_rtree_info(h_, &n, &nl, &numParts, &pml, &partMapType);
        std::vector<float> f(5 * (size_t)n), ld((size_t)nl * numParts);
        std::vector<int> l(3 * (size_t)n);
        leafBestMatch.assign(nl, 0);
        partMap.assign(pml, 0);
        avt_rtree_get(h_, f.data(), l.data(), ld.data(), leafBestMatch.data(), partMap.data());
        nodes.assign(n, RNode());
        for (int i = 0; i < n; ++i) {
            RNode& nd = nodes[i];
            nd.u[0] = f[5 * i]; nd.u[1] = f[5 * i + 1]; nd.v[0] = f[5 * i + 2]; nd.v[1] = f[5 * i + 3]; nd.thresh = f[5 * i + 4];
            nd.lnode = l[3 * i]; nd.rnode = l[3 * i + 1]; nd.leafid = l[3 * i + 2];
        }
        leafData.assign(nl, Distribution());
        for (int i = 0; i < nl; ++i) leafData[i].assign(ld.begin() + (size_t)i * numParts, ld.begin() + (size_t)(i + 1) * numParts);
    }
    avt_rtree_trainer* trainer(int k, int f, int probe, int min_samples, int depth, int T, uint64_t seed) {
        avt_rtree_train_params p{numParts, k, f, (float)probe, min_samples, depth, T, seed};
        avt_rtree_trainer* tr = nullptr;
        if (avt_rtree_trainer_create(device_, &p, &tr) != 0) die("train");
        return tr;
    }
    void finish_training(avt_rtree_trainer* tr, const std::vector<int>& part_map, int part_map_type) {
        avt_rtree* out = nullptr;
        const int rc = avt_rtree_trainer_run(tr, (int)part_map.size(), part_map.data(), part_map_type, &out, nullptr);
        avt_rtree_trainer_destroy(tr);
        if (rc != 0) die("train");
        avt_rtree_destroy(h_);
        h_ = out;
        pull();
    }
    int device_ = 0;
};

}  // namespace ark
