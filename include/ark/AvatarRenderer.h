// ark/AvatarRenderer.h — `ark::AvatarRenderer` (the reference's AvatarRenderer.h / AvatarRenderer.cpp:11-224) over the C ABI of
// avt_render.h.  The public surface is the reference's: the class name, the (avatar, intrinsics) constructor, the seven methods
// and update().  The images are computed on the GPU and equal the reference's pixel for pixel.  cv::Mat becomes the row-major
// images of ark/RTree.h (ImageF depth, Image8 part mask and Lambert overlay, Image<int32_t> face ids), cv::Point2f becomes
// ark::Point2f and cv::Vec3i a std::array<int, 3>.
//
// The renderer refers to the avatar and the intrinsics it was made with and keeps what it computed (projections, painter order,
// the avatar's cloud on the device) until update() is called.  Call update() after every change of the avatar's state.  The
// device handle is made on first use and made again when the image size changes; a copy starts without one.
#pragma once
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../avt_render.h"
#include "Avatar.h"
#include "RTree.h"

namespace ark {

class AvatarRenderer {
public:
    typedef std::pair<float, std::array<int, 3>> FaceType;

    /** A renderer of `ava` as seen by a camera with intrinsics `intrin` (both are referenced, not copied); `device`: the HIP device. */
    AvatarRenderer(const Avatar& ava, const CameraIntrin& intrin, int device = 0) : avatar_(ava), camera_(intrin), deviceId_(device) {}
    ~AvatarRenderer() { avt_renderer_destroy(gpu_.handle); }
    /** A copy keeps the computed projections and order; it makes its own device handle when it first needs one. */
    AvatarRenderer(const AvatarRenderer& o) : avatar_(o.avatar_), camera_(o.camera_), deviceId_(o.deviceId_), cached_(o.cached_) {}
    /** A move takes the device handle over. */
    AvatarRenderer(AvatarRenderer&& o) noexcept
        : avatar_(o.avatar_), camera_(o.camera_), deviceId_(o.deviceId_), cached_(std::move(o.cached_)), gpu_(o.gpu_) {
        o.gpu_ = GpuState();
    }
    // it refers to an avatar and intrinsics, so it cannot be re-pointed by assignment (the reference's class cannot either)
    AvatarRenderer& operator=(const AvatarRenderer&) = delete;
    AvatarRenderer& operator=(AvatarRenderer&&) = delete;

    /** Pixel position of every vertex of the avatar (AvatarRenderer.cpp:11-24). */
    const std::vector<Point2f>& getProjectedPoints() const {
        if (cached_.points.empty()) {
            cached_.points.resize((size_t)avatar_.model.numPoints());
            if (hasCloud()) computeProjection();
        }
        return cached_.points;
    }

    /** Pixel position of every joint of the avatar (AvatarRenderer.cpp:26-37). */
    const std::vector<Point2f>& getProjectedJoints() const {
        if (cached_.joints.empty()) {
            cached_.joints.resize((size_t)avatar_.model.numJoints());
            if (hasCloud() && avatar_.jointPos.cols() != 0) computeProjection();
        }
        return cached_.joints;
    }

    /** The painter order: (mean vertex depth, vertex ids) of every face, deepest first; equal depths in face id order
     *  (AvatarRenderer.cpp:39-70). */
    const std::vector<FaceType>& getOrderedFaces() const {
        if (cached_.faces.empty()) {
            if (!hasCloud()) {
                const int F = avatar_.model.numFaces();
                cached_.faces.reserve((size_t)F);
                for (int f = 0; f < F; ++f)
                    cached_.faces.emplace_back(0.f, std::array<int, 3>{avatar_.model.mesh(0, f), avatar_.model.mesh(1, f), avatar_.model.mesh(2, f)});
                noCloudWarning();
                return cached_.faces;
            }
            computeProjection();
        }
        return cached_.faces;
    }

    /** Float depth image; 0 where no face is painted (AvatarRenderer.cpp:72-101). */
    ImageF renderDepth(const Size& image_size) const {
        if (!hasCloud()) { noCloudWarning(); return ImageF(); }
        ImageF img(image_size.height, image_size.width);
        runOn(image_size, AVT_RENDER_DEPTH, nullptr);
        check(avt_renderer_download(gpu_.handle, 0, img.data(), nullptr, nullptr, nullptr), "renderDepth");
        return img;
    }

    /** 8-bit diffuse shading under the reference's two lights; 0 where no face is painted (AvatarRenderer.cpp:104-172). */
    Image8 renderLambert(const Size& image_size) const {
        if (!hasCloud()) { noCloudWarning(); return Image8(); }
        Image8 img(image_size.height, image_size.width);
        runOn(image_size, AVT_RENDER_LAMBERT, nullptr);
        check(avt_renderer_download(gpu_.handle, 0, nullptr, nullptr, img.data(), nullptr), "renderLambert");
        return img;
    }

    /** Body part of every pixel, 255 where no face is painted.  part_map[j] is the part of joint j; an empty map labels
     *  pixels with the joint id (AvatarRenderer.cpp:174-202). */
    Image8 renderPartMask(const Size& image_size, const std::vector<int>& part_map = {}) const {
        if (!hasCloud()) { noCloudWarning(); return Image8(); }
        Image8 img(image_size.height, image_size.width);
        runOn(image_size, AVT_RENDER_PART_MASK, &part_map);
        check(avt_renderer_download(gpu_.handle, 0, nullptr, img.data(), nullptr, nullptr), "renderPartMask");
        return img;
    }

    /** renderDepth and renderPartMask in one run, left on the device for a consumer that reads them there
     *  (RForest::scoreRendered); nothing is downloaded.  False (and a warning) when the avatar has no posed cloud. */
    bool renderDepthAndPartMaskOnDevice(const Size& image_size, const std::vector<int>& part_map = {}) const {
        if (!hasCloud()) { noCloudWarning(); return false; }
        runOn(image_size, AVT_RENDER_DEPTH | AVT_RENDER_PART_MASK, &part_map);
        return true;
    }

    /** The C handle of the last render (null before the first one), for the calls that take over its images on the device. */
    avt_renderer* handle() const { return gpu_.handle; }

    /** Index into getOrderedFaces() of the face painted last at every pixel, -1 where none is (AvatarRenderer.cpp:204-217).
     *  num_threads is accepted for source compatibility and ignored. */
    Image<int32_t> renderFaces(const Size& image_size, int num_threads = 1) const {
        (void)num_threads;
        Image<int32_t> img(image_size.height, image_size.width, -1);
        if (!hasCloud()) { getOrderedFaces(); return img; }     // the reference paints nothing then: every point projects to (0, 0)
        runOn(image_size, AVT_RENDER_FACES, nullptr);
        check(avt_renderer_download(gpu_.handle, 0, nullptr, nullptr, nullptr, img.data()), "renderFaces");
        return img;
    }

    /** Forgets the projections, the painter order and the uploaded cloud: the next call works on the avatar as it is now. */
    void update() const {
        cached_ = Cached();
        gpu_.cloudCurrent = false;
    }

private:
    struct Cached {                    // host copies of what the device computed for the current cloud
        std::vector<Point2f> points, joints;
        std::vector<FaceType> faces;
    };
    struct GpuState {                  // the device handle and what it holds
        avt_renderer* handle = nullptr;
        int width = 0, height = 0;
        bool cloudCurrent = false;
    };

    bool hasCloud() const { return avatar_.cloud.cols() != 0; }
    static void check(int rc, const char* what) {
        if (rc != 0) { std::fprintf(stderr, "AvatarRenderer::%s: %s\n", what, avt_last_error()); std::exit(1); }
    }
    static void noCloudWarning() { std::fprintf(stderr, "WARNING: AvatarRenderer: the avatar has no posed cloud yet (run its update()); nothing rendered\n"); }

    // a handle for images of `size` that holds the avatar's current cloud
    void prepare(const Size& size) const {
        if (!gpu_.handle || size.width != gpu_.width || size.height != gpu_.height) {
            avt_renderer_destroy(gpu_.handle);
            gpu_ = GpuState();
            check(avt_renderer_create(deviceId_, avatar_.model.handle, size.width, size.height, camera_.fx, camera_.fy, camera_.cx, camera_.cy, 1,
                                      &gpu_.handle), "create");
            gpu_.width = size.width;
            gpu_.height = size.height;
        }
        if (!gpu_.cloudCurrent) {
            check(avt_renderer_upload(gpu_.handle, 1, avatar_.cloud.data(), avatar_.jointPos.cols() ? avatar_.jointPos.data() : nullptr), "upload");
            gpu_.cloudCurrent = true;
        }
    }

    void runOn(const Size& size, int what, const std::vector<int>* part_map) const {
        prepare(size);
        if (part_map) check(avt_renderer_set_part_map(gpu_.handle, (int)part_map->size(), part_map->empty() ? nullptr : part_map->data()), "renderPartMask");
        check(avt_renderer_run(gpu_.handle, what), "run");
    }

    // projections and painter order of the current cloud, fetched from the device into the host caches
    void computeProjection() const {
        prepare(gpu_.handle ? Size(gpu_.width, gpu_.height) : Size(1, 1));
        check(avt_renderer_run(gpu_.handle, 0), "run");
        const int V = avatar_.model.numPoints(), J = avatar_.model.numJoints(), F = avatar_.model.numFaces();
        const bool withJoints = avatar_.jointPos.cols() != 0;
        std::vector<float> pv(2 * (size_t)V), pj(2 * (size_t)(J > 0 ? J : 1)), depthKey((size_t)F);
        std::vector<int> ids(3 * (size_t)F);
        check(avt_renderer_projection(gpu_.handle, 0, pv.data(), withJoints ? pj.data() : nullptr, depthKey.data(), ids.data(), nullptr), "projection");
        cached_.points.assign((size_t)V, Point2f());
        for (size_t i = 0; i < (size_t)V; ++i) cached_.points[i] = Point2f{pv[2 * i], pv[2 * i + 1]};
        cached_.joints.assign((size_t)J, Point2f());
        if (withJoints) for (size_t i = 0; i < (size_t)J; ++i) cached_.joints[i] = Point2f{pj[2 * i], pj[2 * i + 1]};
        cached_.faces.clear();
        cached_.faces.reserve((size_t)F);
        for (size_t f = 0; f < (size_t)F; ++f) cached_.faces.emplace_back(depthKey[f], std::array<int, 3>{ids[3 * f], ids[3 * f + 1], ids[3 * f + 2]});
    }

    const Avatar& avatar_;
    const CameraIntrin& camera_;
    int deviceId_;
    mutable Cached cached_;
    mutable GpuState gpu_;
};

}  // namespace ark
