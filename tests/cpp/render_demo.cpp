// render_demo.cpp — the overlay line of the reference's demo loop (demo.cpp:179-290: `ark::AvatarRenderer rend(ava, intrin);
// rend.renderLambert(size)`) with the C++ facade, plus the other three images and the cached projections.  Inputs written by
// tests/test_gpu_avatar_render.py:
//   argv[1] model dir (model.npz), argv[2] state.bin (K w, 3 p, J*9 R col-major; int width, int height; 4 float intrinsics),
//   argv[3] output.bin: 3V cloud (double), then renderDepth (float), renderPartMask, renderLambert (uint8), renderFaces (int32),
//   getProjectedPoints (2V float), getProjectedJoints (2J float), getOrderedFaces (F float keys, 3F int).
#include <cstdio>
#include <vector>

#include "ark/AvatarRenderer.h"

int main(int argc, char** argv) {
    if (argc < 4) { std::fprintf(stderr, "usage: render_demo model_dir state.bin out.bin\n"); return 2; }
    const ark::AvatarModel model(argv[1]);
    ark::Avatar ava(model);
    const int J = model.numJoints(), K = model.numShapeKeys();
    FILE* f = std::fopen(argv[2], "rb");
    if (!f) { std::perror("state"); return 2; }
    bool ok = std::fread(ava.w.data(), sizeof(double), K, f) == (size_t)K && std::fread(ava.p.data(), sizeof(double), 3, f) == 3;
    for (int j = 0; ok && j < J; ++j) ok = std::fread(ava.r[j].data(), sizeof(double), 9, f) == 9;
    int size[2] = {0, 0};
    ark::CameraIntrin intrin;
    ok = ok && std::fread(size, sizeof(int), 2, f) == 2 && std::fread(&intrin.fx, sizeof(float), 1, f) == 1 &&
         std::fread(&intrin.fy, sizeof(float), 1, f) == 1 && std::fread(&intrin.cx, sizeof(float), 1, f) == 1 &&
         std::fread(&intrin.cy, sizeof(float), 1, f) == 1;
    std::fclose(f);
    if (!ok) { std::fprintf(stderr, "short state file\n"); return 2; }

    ark::AvatarRenderer rend(ava, intrin);
    const ark::Size imsize(size[0], size[1]);
    const ark::ImageF empty = rend.renderDepth(imsize);          // before update(): the reference warns and returns an empty image
    if (!empty.a.empty()) { std::fprintf(stderr, "an empty avatar rendered an image\n"); return 1; }
    ava.update();
    rend.update();

    const ark::Image8 lambert = rend.renderLambert(imsize);       // the demo loop's overlay
    const ark::ImageF depth = rend.renderDepth(imsize);
    const ark::Image8 mask = rend.renderPartMask(imsize);
    const ark::Image<int32_t> faces = rend.renderFaces(imsize);
    const auto& pts = rend.getProjectedPoints();
    const auto& jts = rend.getProjectedJoints();
    const auto& ord = rend.getOrderedFaces();

    FILE* o = std::fopen(argv[3], "wb");
    if (!o) { std::perror("out"); return 2; }
    std::fwrite(ava.cloud.data(), sizeof(double), ava.cloud.size(), o);
    std::fwrite(depth.data(), sizeof(float), depth.a.size(), o);
    std::fwrite(mask.data(), 1, mask.a.size(), o);
    std::fwrite(lambert.data(), 1, lambert.a.size(), o);
    std::fwrite(faces.data(), sizeof(int32_t), faces.a.size(), o);
    for (const auto& p : pts) { std::fwrite(&p.x, sizeof(float), 1, o); std::fwrite(&p.y, sizeof(float), 1, o); }
    for (const auto& p : jts) { std::fwrite(&p.x, sizeof(float), 1, o); std::fwrite(&p.y, sizeof(float), 1, o); }
    for (const auto& fc : ord) std::fwrite(&fc.first, sizeof(float), 1, o);
    for (const auto& fc : ord) std::fwrite(fc.second.data(), sizeof(int), 3, o);
    std::fclose(o);
    int lit = 0;
    for (uint8_t v : lambert.a) lit += v != 0;
    std::printf("render_demo: %dx%d, %d lit overlay pixels\n", size[0], size[1], lit);
    return 0;
}
