// occlusion_demo.cpp — ark::AvatarOptimizer::renderOcclusion through the C++ facade (tests/test_gpu_occlusion.py).
//   argv[1] model dir (model.npz + pose_prior.txt), argv[2] frame.bin in facade_demo's format (int N; N*3 doubles xyz; N ints labels;
//   start state: 10 w, 3 p, 24*9 R col-major).
// One ICP iteration from the same start state with the back-face test alone and with the face-id render on top of it (the optimizer's
// own intrin and imageSize): the second must leave fewer visible vertices, and none that the first hides.
#include <cstdio>
#include <vector>

#include "ark/AvatarOptimizer.h"

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: occlusion_demo model_dir frame.bin\n"); return 2; }
    const ark::AvatarModel model(argv[1]);
    ark::Avatar ava(model);
    FILE* f = std::fopen(argv[2], "rb");
    if (!f) { std::perror("frame"); return 2; }
    int N = 0;
    if (std::fread(&N, sizeof(int), 1, f) != 1) return 2;
    ark::CloudType dataCloud;
    dataCloud.resize(3, N);
    ark::VectorXi labels(N);
    const int J = model.numJoints(), K = model.numShapeKeys();
    bool okr = std::fread(dataCloud.data(), sizeof(double), 3 * (size_t)N, f) == 3 * (size_t)N &&
               std::fread(labels.data(), sizeof(int), N, f) == (size_t)N &&
               std::fread(ava.w.data(), sizeof(double), K, f) == (size_t)K && std::fread(ava.p.data(), sizeof(double), 3, f) == 3;
    for (int j = 0; okr && j < J; ++j) okr = std::fread(ava.r[j].data(), sizeof(double), 9, f) == 9;
    std::fclose(f);
    if (!okr) { std::fprintf(stderr, "short frame file\n"); return 2; }
    const auto w0 = ava.w;
    const auto p0 = ava.p;
    const auto r0 = ava.r;

    ark::CameraIntrin intrin;                                  // the reference's defaults: the K4A camera the frame was rendered with
    std::vector<int> partMap(J);
    for (int j = 0; j < J; ++j) partMap[j] = j;
    ark::AvatarOptimizer avaOpt(ava, intrin, ark::Size(1280, 720), J, partMap);
    avaOpt.maxItersPerICP = 0;
    std::vector<unsigned char> vis[2];
    for (int on = 0; on < 2; ++on) {
        ava.w = w0; ava.p = p0; ava.r = r0;
        ava.update();
        avaOpt.renderOcclusion = on != 0;
        avaOpt.optimize(dataCloud, labels, 1, 4);
        vis[on] = avaOpt.visibility();
    }
    long n[2] = {0, 0}, outside = 0;
    for (size_t v = 0; v < vis[0].size(); ++v) {
        n[0] += vis[0][v]; n[1] += vis[1][v];
        if (vis[1][v] && !vis[0][v]) ++outside;
    }
    std::printf("occlusion_demo: %ld visible by the back-face test, %ld with the render, %ld of them not in the first set\n", n[0], n[1], outside);
    if (!(n[1] < n[0]) || outside != 0) { std::printf("occlusion_demo FAILED\n"); return 1; }
    std::printf("occlusion_demo ok\n");
    return 0;
}
