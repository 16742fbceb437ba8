// rtree_train_demo.cpp — forest training through the C++ facade (include/ark/RTree.h), the way `rtree-train` uses the
// reference's class: train, then exportFile.  Used by tests/test_gpu_rtree_train.py.
//   rtree_train_demo images <images.bin> <out.srtr> P k F probe min_samples depth T seed
//       images.bin: int32 n, rows, cols, then n x rows x cols float32 depth, then n x rows x cols uint8 part masks
//       -> ark::RTree(P).train(depth, masks, ...) -> exportFile
//   rtree_train_demo avatar <model_dir> <out.srtr> <images_out.bin> n width height k F probe min_samples depth T seed batch
//       -> ark::RTree(J).trainFromAvatar(model, intrin, size, ...) -> exportFile, and the same avatars rendered through
//          ark::Avatar::update + ark::AvatarRenderer (renderDepth / renderPartMask) written to images_out.bin
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ark/AvatarRenderer.h"
#include "ark/RTree.h"

static int images_mode(char** a) {
    FILE* f = std::fopen(a[2], "rb");
    if (!f) return 2;
    int hdr[3];
    if (std::fread(hdr, sizeof(int), 3, f) != 3) return 2;
    const int n = hdr[0], rows = hdr[1], cols = hdr[2];
    std::vector<ark::ImageF> depth(n, ark::ImageF(rows, cols));
    std::vector<ark::Image8> mask(n, ark::Image8(rows, cols));
    for (auto& d : depth) if (std::fread(d.data(), sizeof(float), (size_t)rows * cols, f) != (size_t)rows * cols) return 2;
    for (auto& m : mask) if (std::fread(m.data(), 1, (size_t)rows * cols, f) != (size_t)rows * cols) return 2;
    std::fclose(f);
    ark::RTree rtree(std::atoi(a[4]));
    rtree.train(depth, mask, 0, false, std::atoi(a[5]), std::atoi(a[6]), std::atoi(a[7]), std::atoi(a[8]), std::atoi(a[9]), std::atoi(a[10]),
                std::strtoull(a[11], nullptr, 10));
    std::printf("trained: %zu nodes, %zu leaves\n", rtree.nodes.size(), rtree.leafData.size());
    return rtree.exportFile(a[3]) ? 0 : 1;
}

static int avatar_mode(char** a) {
    ark::AvatarModel model(a[2]);
    const int n = std::atoi(a[5]), W = std::atoi(a[6]), H = std::atoi(a[7]);
    const uint64_t seed = std::strtoull(a[14], nullptr, 10);
    const ark::CameraIntrin intrin;
    const ark::Size size(W, H);
    // Avatar::randomize's pose comes from the library's own generators, which a seed does not pin (Avatar.h): reseed them so
    // that the host loop below draws the same avatars as trainFromAvatar
    ark::random_util::reseed(12345u);
    ark::RTree rtree(model.numJoints());
    rtree.trainFromAvatar(model, intrin, size, 0, false, n, std::atoi(a[8]), std::atoi(a[9]), 200, std::atoi(a[10]), std::atoi(a[11]),
                          std::atoi(a[12]), std::atoi(a[13]), 0.01f, 15, {}, 50, 12000, "", seed, std::atoi(a[15]));
    std::printf("trainFromAvatar: %zu nodes, %zu leaves\n", rtree.nodes.size(), rtree.leafData.size());
    if (!rtree.exportFile(a[3])) return 1;
    // the same avatars through the host-facing classes: Avatar::update, AvatarRenderer::renderDepth / renderPartMask
    FILE* f = std::fopen(a[4], "wb");
    if (!f) return 2;
    const int hdr[3] = {n, H, W};
    std::fwrite(hdr, sizeof(int), 3, f);
    ark::random_util::reseed(12345u);
    ark::Avatar ava(model);
    ark::AvatarRenderer rend(ava, intrin);
    std::vector<ark::Image8> masks;
    const uint32_t xorKey = avt_rt_xor_key(seed);
    for (int idx = 0; idx < n; ++idx) {
        ava.randomize(true, true, true, (uint32_t)idx ^ xorKey);
        ava.update();
        rend.update();
        const ark::ImageF d = rend.renderDepth(size);
        std::fwrite(d.data(), sizeof(float), (size_t)W * H, f);
        masks.push_back(rend.renderPartMask(size));
    }
    for (auto& m : masks) std::fwrite(m.data(), 1, (size_t)W * H, f);
    std::fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 12 && std::strcmp(argv[1], "images") == 0) return images_mode(argv);
    if (argc == 16 && std::strcmp(argv[1], "avatar") == 0) return avatar_mode(argv);
    std::fprintf(stderr, "usage: see the head of rtree_train_demo.cpp\n");
    return 2;
}
