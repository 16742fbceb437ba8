// multi_render_demo.cpp — ark::MultiFrameTracker::render: one step of S streams, then the overlays of some of them rendered on the
// device from the tracker's context (no cloud download), read back with renderedDepth / PartMask / Lambert / Faces.
//   argv[1] model dir (model.npz)
//   argv[2] output.bin: per rendered stream: 3V cloud, 3J joint positions (double, from posed()), then depth (float), part mask,
//           Lambert (uint8), faces (int32), each height x width
//   argv[3] width, argv[4] height, argv[5] the rendered streams, comma separated (e.g. "2,0")
//   argv[6..] one sequence file per stream in tracker_demo's format (tests/test_gpu_tracker.py write_sequence); frame 0 is used
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <string>
#include <vector>

#include "ark/MultiFrameTracker.h"

int main(int argc, char** argv) {
    if (argc < 7) { std::fprintf(stderr, "usage: multi_render_demo model_dir out.bin width height s0,s1,.. seq.bin [seq.bin ...]\n"); return 2; }
    const ark::AvatarModel model(argv[1]);
    const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), S = argc - 6;
    std::vector<int> streams;
    {
        std::stringstream ss(argv[5]);
        std::string item;
        while (std::getline(ss, item, ',')) streams.push_back(std::atoi(item.c_str()));
    }
    std::vector<std::vector<float>> xyz((size_t)S);
    std::vector<std::vector<std::uint8_t>> mask((size_t)S);
    std::vector<ark::MultiFrameTracker::Frame> frames((size_t)S);
    int hdr[7] = {0};
    for (int s = 0; s < S; ++s) {
        FILE* f = std::fopen(argv[6 + s], "rb");
        if (!f) { std::perror("sequence"); return 2; }
        int b[4];
        bool ok = std::fread(hdr, sizeof(int), 7, f) == 7;
        const size_t n = (size_t)hdr[1] * hdr[2];
        xyz[(size_t)s].resize(3 * n);
        mask[(size_t)s].resize(n);
        ok = ok && std::fread(b, sizeof(int), 4, f) == 4 && std::fread(xyz[(size_t)s].data(), sizeof(float), 3 * n, f) == 3 * n &&
             std::fread(mask[(size_t)s].data(), 1, n, f) == n;
        std::fclose(f);
        if (!ok) { std::fprintf(stderr, "short sequence file\n"); return 2; }
        ark::MultiFrameTracker::Frame& fr = frames[(size_t)s];
        fr.xyz = xyz[(size_t)s].data(); fr.mask = mask[(size_t)s].data(); fr.width = hdr[1]; fr.height = hdr[2];
        fr.box.top = b[0]; fr.box.left = b[1]; fr.box.bottom = b[2]; fr.box.right = b[3];
    }
    const int J = model.numJoints(), V = model.numPoints();
    std::vector<int> partMap((size_t)J);
    for (int j = 0; j < J; ++j) partMap[(size_t)j] = j;
    int maxPts = 1;
    for (int r = 0; r < hdr[2]; r += hdr[3]) for (int c = 0; c < hdr[1]; c += hdr[3]) ++maxPts;
    ark::MultiFrameTracker tracker(model, S, J, partMap, maxPts);
    for (auto& st : tracker.streams) { st.interval = hdr[3]; st.frameICPIters = hdr[4]; st.reinitICPIters = st.initialICPIters = hdr[5]; st.reinitCnz = hdr[6]; }
    std::vector<int> fitted;
    tracker.process(frames, fitted);
    for (int s : streams) if (!fitted[(size_t)s]) { std::fprintf(stderr, "stream %d was not fitted\n", s); return 1; }

    ark::CameraIntrin intrin;
    intrin.fx = 0.5f * W; intrin.fy = 0.5f * W; intrin.cx = 0.5f * W - 0.5f; intrin.cy = 0.5f * H + 0.25f;
    tracker.render(streams, ark::Size(W, H), intrin, AVT_RENDER_DEPTH | AVT_RENDER_PART_MASK | AVT_RENDER_LAMBERT | AVT_RENDER_FACES);
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) { std::perror("out"); return 2; }
    std::vector<double> cloud(3 * (size_t)V), joints(3 * (size_t)J);
    for (size_t i = 0; i < streams.size(); ++i) {
        tracker.posed(streams[i], cloud.data(), joints.data());
        const ark::ImageF depth = tracker.renderedDepth((int)i);
        const ark::Image8 parts = tracker.renderedPartMask((int)i), lambert = tracker.renderedLambert((int)i);
        const ark::Image<int32_t> faces = tracker.renderedFaces((int)i);
        std::fwrite(cloud.data(), sizeof(double), cloud.size(), o);
        std::fwrite(joints.data(), sizeof(double), joints.size(), o);
        std::fwrite(depth.data(), sizeof(float), depth.a.size(), o);
        std::fwrite(parts.data(), 1, parts.a.size(), o);
        std::fwrite(lambert.data(), 1, lambert.a.size(), o);
        std::fwrite(faces.data(), sizeof(int32_t), faces.a.size(), o);
    }
    std::fclose(o);
    std::printf("multi_render_demo: %d streams, %d rendered at %dx%d\n", S, (int)streams.size(), W, H);
    return 0;
}
