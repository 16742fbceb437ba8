// fit_score_demo.cpp — the fit score through the C++ facade (ark/FitScore.h, ark::MultiFrameTracker::fitScore, ark::fitLost).
//   fit_score_demo derive in.bin out.bin
//       in:  int32 P; (P + 1) x 7 int64 table; float64 minIoU, maxViolation
//       out: float64 iou agree violation unexplained meanAbsErr meanAbsErrAgree of the whole table, the same six of every row,
//            agree / violation / meanAbsErr / meanAbsErrAgree of every row again through the per-part accessors, then fitLost
//            as 0.0 / 1.0.  Runs without a GPU.
//   fit_score_demo images in.bin out.bin
//       in:  int32 n, rows, cols, P, stride, has_boxes; float32 tol; n x rows x cols float32 R, uint8 M, float32 D; n x 4 int32
//       out: n x (P + 1) x 7 int64 through ark::FitScorer::score
//   fit_score_demo tracker model_dir forest in.bin out.bin
//       in:  int32 S, steps, rows, cols, data interval, frame ICP iters, reinit ICP iters, min points, forest interval, stride;
//            float32 nnDistThreshRel, neighbThreshRel, tol; S cameras (fx fy cx cy float32); S background depth images; steps x S
//            depth images
//       out: per step S int32 fitted, then the S tables of fitScore for the streams in DESCENDING order (a permuted obs_index),
//            rendered with camera 0 at cols x rows
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ark/MultiFrameTracker.h"

static void put(FILE* o, const ark::FitFigures& f) {
    const double v[6] = {f.iou, f.agree, f.violation, f.unexplained, f.meanAbsErr, f.meanAbsErrAgree};
    std::fwrite(v, sizeof(double), 6, o);
}

static int derive_mode(const char* in, const char* out) {
    FILE* f = std::fopen(in, "rb");
    if (!f) { std::perror("input"); return 2; }
    int P = 0;
    if (std::fread(&P, sizeof(int), 1, f) != 1) return 2;
    ark::FitScore s;
    s.numParts = P;
    s.table.resize((size_t)(P + 1) * AVT_FITSCORE_COLS);
    double bounds[2];
    if (std::fread(s.table.data(), sizeof(long long), s.table.size(), f) != s.table.size() || std::fread(bounds, sizeof(double), 2, f) != 2) return 2;
    std::fclose(f);
    FILE* o = std::fopen(out, "wb");
    if (!o) { std::perror("output"); return 2; }
    put(o, s.derive());
    for (int p = 0; p <= P; ++p) put(o, s.derive(p));
    for (int p = 0; p <= P; ++p) {
        const double v[4] = {s.agree(p), s.violation(p), s.meanAbsErr(p), s.meanAbsErrAgree(p)};
        std::fwrite(v, sizeof(double), 4, o);
    }
    const double lost = ark::fitLost(s, bounds[0], bounds[1]) ? 1.0 : 0.0;
    std::fwrite(&lost, sizeof(double), 1, o);
    std::fclose(o);
    return 0;
}

static void put_tables(FILE* o, const std::vector<ark::FitScore>& scores) {
    for (const ark::FitScore& s : scores) std::fwrite(s.table.data(), sizeof(long long), s.table.size(), o);
}

static int images_mode(const char* in, const char* out) {
    FILE* f = std::fopen(in, "rb");
    if (!f) { std::perror("input"); return 2; }
    int h[6];
    float tol;
    if (std::fread(h, sizeof(int), 6, f) != 6 || std::fread(&tol, sizeof(float), 1, f) != 1) return 2;
    const int n = h[0], rows = h[1], cols = h[2], P = h[3], stride = h[4];
    std::vector<ark::ImageF> R((size_t)n, ark::ImageF(rows, cols)), D((size_t)n, ark::ImageF(rows, cols));
    std::vector<ark::Image8> M((size_t)n, ark::Image8(rows, cols));
    const size_t px = (size_t)rows * cols;
    for (auto& im : R) if (std::fread(im.data(), sizeof(float), px, f) != px) return 2;
    for (auto& im : M) if (std::fread(im.data(), 1, px, f) != px) return 2;
    for (auto& im : D) if (std::fread(im.data(), sizeof(float), px, f) != px) return 2;
    std::vector<std::array<int, 4>> boxes(h[5] ? (size_t)n : 0);
    for (auto& b : boxes) if (std::fread(b.data(), sizeof(int), 4, f) != 4) return 2;
    std::fclose(f);
    ark::FitScorer scorer(P, n);
    FILE* o = std::fopen(out, "wb");
    if (!o) { std::perror("output"); return 2; }
    put_tables(o, scorer.score(R, M, D, boxes, tol, stride));
    std::fclose(o);
    return 0;
}

static int tracker_mode(char** argv) {
    const ark::AvatarModel model(argv[2]);
    const std::string forest(argv[3]);
    ark::RTree tree(forest);
    FILE* f = std::fopen(argv[4], "rb");
    if (!f) { std::perror("input"); return 2; }
    int h[10];
    float rel[3];
    if (std::fread(h, sizeof(int), 10, f) != 10 || std::fread(rel, sizeof(float), 3, f) != 3) return 2;
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
    const int J = model.numJoints();
    std::vector<int> partMap(J);
    for (int j = 0; j < J; ++j) partMap[j] = j;
    ark::MultiFrameTracker tracker(model, S, J, partMap, rows * cols / (h[4] * h[4]) + 1);
    tracker.betaPose = 0.05;      // demo.cpp:139-143
    tracker.betaShape = 0.12;
    for (auto& st : tracker.streams) {
        st.interval = h[4]; st.frameICPIters = h[5]; st.reinitICPIters = st.initialICPIters = h[6]; st.reinitCnz = h[7];
    }
    tracker.attachFrontEnd(bgsub, tree, h[8]);
    FILE* o = std::fopen(argv[5], "wb");
    if (!o) { std::perror("output"); return 2; }
    std::vector<int> fitted, order;
    for (int s = S - 1; s >= 0; --s) order.push_back(s);
    for (int t = 0; t < steps; ++t) {
        read_images(images);
        tracker.processDepthImages(images, cams, fitted);
        std::fwrite(fitted.data(), sizeof(int), (size_t)S, o);
        put_tables(o, tracker.fitScore(order, ark::Size(cols, rows), cams[0], rel[2], h[9], partMap));
    }
    std::fclose(o);
    std::fclose(f);
    std::printf("fit_score_demo: %d streams, %d steps\n", S, steps);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && !std::strcmp(argv[1], "derive")) return derive_mode(argv[2], argv[3]);
    if (argc == 4 && !std::strcmp(argv[1], "images")) return images_mode(argv[2], argv[3]);
    if (argc == 6 && !std::strcmp(argv[1], "tracker")) return tracker_mode(argv);
    std::fprintf(stderr, "usage: fit_score_demo derive in out | images in out | tracker model_dir forest in out\n");
    return 2;
}
