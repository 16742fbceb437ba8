// multi_subsample_demo.cpp — multi_depth_demo's counterpart with the whole front end on the device: S streams through
// ark::MultiFrameTracker::processDepthImages with devicePostProcess and deviceSubsample (include/avt_subsample.h): the labels are
// post-processed where they lie, the kept points go straight into the context's frame slots, the policy runs on the table of counts
// (ark::frameDecision on a count row) and avt_frames_subsample_commit makes the frames resident.
//   argv[1] model dir (model.npz + pose_prior.txt)
//   argv[2] forest file
//   argv[3] input.bin: int32 S, steps, rows, cols, data interval, frame ICP iters, reinit ICP iters, min points, forest interval;
//           float32 nnDistThreshRel, neighbThreshRel; S cameras (fx fy cx cy float32); S background depth images (rows x cols
//           float32); steps x S depth images
//   argv[4] output.bin: per step S x rows x cols label bytes (downloadPartMasks), S x 4 int32 boxes (tl.x tl.y br.x br.y), S int32
//           fitted, S int32 budgets, then 3 S doubles p, 4 J S q (x, y, z, w), K S w
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ark/MultiFrameTracker.h"

int main(int argc, char** argv) {
    if (argc < 5) { std::fprintf(stderr, "usage: multi_subsample_demo model_dir forest in.bin out.bin\n"); return 2; }
    const ark::AvatarModel model(argv[1]);
    const std::string forest(argv[2]);
    ark::RTree tree(forest);
    FILE* f = std::fopen(argv[3], "rb");
    if (!f) { std::perror("input"); return 2; }
    int h[9];
    float rel[2];
    if (std::fread(h, sizeof(int), 9, f) != 9 || std::fread(rel, sizeof(float), 2, f) != 2) return 2;
    const int S = h[0], steps = h[1], rows = h[2], cols = h[3];
    std::vector<ark::CameraIntrin> cams((size_t)S);
    for (ark::CameraIntrin& k : cams) {
        float v[4];
        if (std::fread(v, sizeof(float), 4, f) != 4) return 2;
        k.fx = v[0]; k.fy = v[1]; k.cx = v[2]; k.cy = v[3];
    }
    auto read_images = [&](std::vector<ark::ImageDepth>& v) {
        v.assign((size_t)S, ark::ImageDepth(rows, cols));
        for (ark::ImageDepth& im : v)
            if (std::fread(im.data(), sizeof(float), im.a.size(), f) != im.a.size()) { std::fprintf(stderr, "short input file\n"); std::exit(2); }
    };
    std::vector<ark::ImageDepth> images;
    read_images(images);
    std::vector<ark::ImageXYZ> backgrounds;
    for (int s = 0; s < S; ++s) backgrounds.push_back(cams[(size_t)s].depthToXYZ(images[(size_t)s]));
    ark::BGSubtractor bgsub(backgrounds);
    bgsub.nnDistThreshRel = rel[0];
    bgsub.neighbThreshRel = rel[1];
    const int J = model.numJoints(), K = model.numShapeKeys();
    std::vector<int> partMap(J);
    for (int j = 0; j < J; ++j) partMap[j] = j;
    ark::MultiFrameTracker tracker(model, S, J, partMap, rows * cols / (h[4] * h[4]) + 1);
    tracker.betaPose = 0.05;      // demo.cpp:139-143
    tracker.betaShape = 0.12;
    for (auto& st : tracker.streams) {
        st.interval = h[4]; st.frameICPIters = h[5]; st.reinitICPIters = st.initialICPIters = h[6]; st.reinitCnz = h[7];
    }
    tracker.attachFrontEnd(bgsub, tree, h[8], 0.001, true, true);
    FILE* o = std::fopen(argv[4], "wb");
    if (!o) { std::perror("output"); return 2; }
    std::vector<int> fitted;
    long fit = 0;
    for (int t = 0; t < steps; ++t) {
        read_images(images);
        tracker.processDepthImages(images, cams, fitted);
        if (!tracker.partMasks.empty()) { std::fprintf(stderr, "a device step left part masks on the host\n"); return 1; }
        const std::vector<ark::Image8>& masks = tracker.downloadPartMasks();
        for (int s = 0; s < S; ++s) std::fwrite(masks[(size_t)s].data(), 1, (size_t)rows * cols, o);
        for (int s = 0; s < S; ++s) std::fwrite(tracker.boxes[(size_t)s].data(), sizeof(int), 4, o);
        std::fwrite(fitted.data(), sizeof(int), (size_t)S, o);
        std::fwrite(tracker.budgets.data(), sizeof(int), (size_t)S, o);
        std::fwrite(tracker.pos(0), sizeof(double), 3 * (size_t)S, o);
        std::fwrite(tracker.quats(0), sizeof(double), 4 * (size_t)J * S, o);
        std::fwrite(tracker.shape(0), sizeof(double), (size_t)K * S, o);
        for (int v : fitted) fit += v;
    }
    std::fclose(o);
    std::fclose(f);
    std::printf("multi_subsample_demo: %d streams, %d steps, %ld fitted\n", S, steps, fit);
    return 0;
}
