// rforest_score_demo.cpp — the comparison rtree-run-dataset leaves to the eye (its `m` key shows the part mask beside the
// arg-max image), in numbers, through the C++ facade (ark/RForest.h).  Used by tests/test_gpu_rforest_score.py.
//   rforest_score_demo <in.bin> <out.bin> tree [tree ...]
//       RForest::score in two calls + scoreGet.  in.bin: int rows, cols, n, stride; n*rows*cols floats of depth; n*rows*cols mask
//       bytes.  out.bin: (numParts+1)^2 long long conf, then numImages, numPixels, missed, spurious as long long, then accuracy,
//       meanIoU and numParts each of recall, precision, iou as doubles.  The trees in forest order.
//   rforest_score_demo avatar <model_dir> <out.bin> width height num_images first_image seed stride tree [tree ...]
//       RForest::scoreFromAvatar in batches of 2 and of 5, and the same avatars through ark::Avatar::update +
//       AvatarRenderer::renderDepthAndPartMaskOnDevice + RForest::scoreRendered: the three matrices must be equal (exit 1
//       otherwise); out.bin as above.
#include <cstdlib>
#include <cstring>
#include <cstdio>
#include <string>
#include <vector>

#include "ark/RForest.h"

static int write_score(const char* path, const ark::RForest& forest, const ark::ForestScore& s) {
    FILE* o = std::fopen(path, "wb");
    if (!o) { std::perror("out"); return 2; }
    const long long tail[4] = {s.numImages, s.numPixels, s.missed, s.spurious};
    const double head[2] = {s.accuracy, s.meanIoU};
    std::fwrite(s.confusion.data(), sizeof(long long), s.confusion.size(), o);
    std::fwrite(tail, sizeof(long long), 4, o);
    std::fwrite(head, sizeof(double), 2, o);
    std::fwrite(s.recall.data(), sizeof(double), s.recall.size(), o);
    std::fwrite(s.precision.data(), sizeof(double), s.precision.size(), o);
    std::fwrite(s.iou.data(), sizeof(double), s.iou.size(), o);
    std::fclose(o);
    std::printf("rforest_score_demo: %d trees, %d parts, %lld images, %lld pixels, accuracy %.4f, mean IoU %.4f, missed %lld, spurious %lld\n",
                forest.numTrees, forest.numParts, s.numImages, s.numPixels, s.accuracy, s.meanIoU, s.missed, s.spurious);
    return 0;
}

static int avatar_mode(int argc, char** a) {
    ark::AvatarModel model(a[2]);
    const int W = std::atoi(a[4]), H = std::atoi(a[5]), n = std::atoi(a[6]), first = std::atoi(a[7]), stride = std::atoi(a[9]);
    const uint64_t seed = std::strtoull(a[8], nullptr, 10);
    ark::CameraIntrin intrin;                     // the default camera, scaled from 1280 x 720 to the image size
    intrin.fx *= W / 1280.f; intrin.cx *= W / 1280.f; intrin.fy *= H / 720.f; intrin.cy *= H / 720.f;
    const ark::Size size(W, H);
    ark::RForest forest(std::vector<std::string>(a + 10, a + argc));
    // Avatar::randomize's pose comes from the library's own generators, which a seed does not pin (Avatar.h): reseed them so
    // that every loop below draws the same avatars
    ark::random_util::reseed(12345u);
    const ark::ForestScore two = forest.scoreFromAvatar(model, intrin, size, n, first, {}, seed, 2, stride);
    ark::random_util::reseed(12345u);
    const ark::ForestScore five = forest.scoreFromAvatar(model, intrin, size, n, first, {}, seed, 5, stride);
    ark::random_util::reseed(12345u);
    ark::Avatar ava(model);
    ark::AvatarRenderer rend(ava, intrin);
    const uint32_t xorKey = avt_rt_xor_key(seed);
    forest.scoreReset();
    for (int idx = first; idx < first + n; ++idx) {
        ava.randomize(true, true, true, (uint32_t)idx ^ xorKey);
        ava.update();
        rend.update();
        if (!rend.renderDepthAndPartMaskOnDevice(size)) return 1;
        forest.scoreRendered(rend, stride);
    }
    const ark::ForestScore byHand = forest.scoreGet();
    if (two.confusion != five.confusion || two.confusion != byHand.confusion || two.numImages != n || five.numImages != n || byHand.numImages != n ||
        two.numPixels != byHand.numPixels) {
        std::fprintf(stderr, "rforest_score_demo: the matrices of batch 2, batch 5 and the host-posed avatars differ\n");
        return 1;
    }
    return write_score(a[3], forest, two);
}

int main(int argc, char** argv) {
    if (argc >= 11 && std::strcmp(argv[1], "avatar") == 0) return avatar_mode(argc, argv);
    if (argc < 4) { std::fprintf(stderr, "usage: see the head of rforest_score_demo.cpp\n"); return 2; }
    ark::RForest forest(std::vector<std::string>(argv + 3, argv + argc));
    if (forest.numParts <= 0) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror("in"); return 2; }
    int hdr[4];
    if (std::fread(hdr, sizeof(int), 4, f) != 4 || hdr[2] < 1) return 2;
    const int rows = hdr[0], cols = hdr[1], n = hdr[2], stride = hdr[3];
    std::vector<ark::ImageF> depth((size_t)n, ark::ImageF(rows, cols));
    std::vector<ark::Image8> mask((size_t)n, ark::Image8(rows, cols));
    for (ark::ImageF& d : depth)
        if (std::fread(d.data(), sizeof(float), d.a.size(), f) != d.a.size()) return 2;
    for (ark::Image8& m : mask)
        if (std::fread(m.data(), 1, m.a.size(), f) != m.a.size()) return 2;
    std::fclose(f);
    // the first image in a call of its own, the others in a second one: the totals add up
    forest.scoreReset();
    forest.score({depth[0]}, {mask[0]}, stride);
    if (n > 1) forest.score(std::vector<ark::ImageF>(depth.begin() + 1, depth.end()), std::vector<ark::Image8>(mask.begin() + 1, mask.end()), stride);
    const ark::ForestScore s = forest.scoreGet();
    return write_score(argv[2], forest, s);
}
