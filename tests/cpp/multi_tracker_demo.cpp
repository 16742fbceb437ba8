// multi_tracker_demo.cpp — S tracking streams through ark::MultiFrameTracker (one batched fit per step).
//   argv[1] model dir (model.npz + pose_prior.txt)
//   argv[2] output.bin: per step, per stream: int fitted; if fitted 3V doubles cloud, 3 p, 4J q (x, y, z, w), K w
//   argv[3] S streams
//   argv[4] timing repeats (0: none): steps 1 .. n-1 of the sequences are replayed that many times
//   argv[5] 1: the timed steps also download every fitted stream's posed cloud, 0: parameters only
//   argv[6] AvatarOptimizer::functionTolerance (< 0: the default 1e-4)
//   argv[7..] sequence files in tracker_demo's format (tests/test_gpu_tracker.py write_sequence; same frame count, size and policy
//             header): stream s plays file s mod nfiles, starting (s / nfiles) frames in (cyclically)
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ark/MultiFrameTracker.h"

struct Seq { std::vector<ark::TrackRect> box; std::vector<std::vector<float>> xyz; std::vector<std::vector<std::uint8_t>> mask; };

int main(int argc, char** argv) {
    if (argc < 8) { std::fprintf(stderr, "usage: multi_tracker_demo model_dir out.bin S repeats posed ftol seq.bin [seq.bin ...]\n"); return 2; }
    const ark::AvatarModel model(argv[1]);
    const int S = std::atoi(argv[3]), reps = std::atoi(argv[4]), posedTimed = std::atoi(argv[5]);
    const double ftol = std::atof(argv[6]);
    const int nfiles = argc - 7;
    int hdr[7] = {0};
    std::vector<Seq> seqs((size_t)nfiles);
    for (int i = 0; i < nfiles; ++i) {
        FILE* f = std::fopen(argv[7 + i], "rb");
        if (!f) { std::perror("sequence"); return 2; }
        int h[7];
        if (std::fread(h, sizeof(int), 7, f) != 7) return 2;
        if (i == 0) std::copy(h, h + 7, hdr);
        else if (h[0] != hdr[0] || h[1] != hdr[1] || h[2] != hdr[2]) { std::fprintf(stderr, "sequences differ in frames / size\n"); return 2; }
        const int W = h[1], H = h[2];
        Seq& sq = seqs[(size_t)i];
        sq.box.resize((size_t)h[0]); sq.xyz.resize((size_t)h[0]); sq.mask.resize((size_t)h[0]);
        for (int t = 0; t < h[0]; ++t) {
            int b[4];
            sq.xyz[(size_t)t].resize((size_t)W * H * 3); sq.mask[(size_t)t].resize((size_t)W * H);
            if (std::fread(b, sizeof(int), 4, f) != 4 || std::fread(sq.xyz[(size_t)t].data(), sizeof(float), sq.xyz[(size_t)t].size(), f) != sq.xyz[(size_t)t].size() ||
                std::fread(sq.mask[(size_t)t].data(), 1, sq.mask[(size_t)t].size(), f) != sq.mask[(size_t)t].size()) { std::fprintf(stderr, "short sequence file\n"); return 2; }
            sq.box[(size_t)t].top = b[0]; sq.box[(size_t)t].left = b[1]; sq.box[(size_t)t].bottom = b[2]; sq.box[(size_t)t].right = b[3];
        }
        std::fclose(f);
    }
    const int nframes = hdr[0], W = hdr[1], H = hdr[2];
    const int J = model.numJoints(), K = model.numShapeKeys(), V = model.numPoints();
    std::vector<int> partMap(J);
    for (int j = 0; j < J; ++j) partMap[j] = j;
    int maxPts = 1;
    for (int r = 0; r < H; r += hdr[3]) for (int c = 0; c < W; c += hdr[3]) ++maxPts;
    ark::MultiFrameTracker tracker(model, S, J, partMap, maxPts);
    tracker.betaPose = 0.05;      // demo.cpp:139-143
    tracker.betaShape = 0.12;
    if (ftol >= 0.0) tracker.functionTolerance = ftol;
    for (auto& st : tracker.streams) {
        st.interval = hdr[3]; st.frameICPIters = hdr[4]; st.reinitICPIters = st.initialICPIters = hdr[5]; st.reinitCnz = hdr[6];
    }
    auto step_frames = [&](int t) {
        std::vector<ark::MultiFrameTracker::Frame> fr((size_t)S);
        for (int s = 0; s < S; ++s) {
            const Seq& sq = seqs[(size_t)(s % nfiles)];
            const size_t k = (size_t)((t + s / nfiles) % nframes);
            fr[(size_t)s] = {sq.xyz[k].data(), sq.mask[k].data(), W, H, sq.box[k]};
        }
        return fr;
    };
    FILE* o = std::fopen(argv[2], "wb");
    std::vector<int> fitted;
    std::vector<double> cloud(3 * (size_t)V);
    for (int t = 0; t < nframes; ++t) {
        tracker.process(step_frames(t), fitted);
        for (int s = 0; s < S; ++s) {
            std::fwrite(&fitted[(size_t)s], sizeof(int), 1, o);
            if (!fitted[(size_t)s]) continue;
            tracker.posed(s, cloud.data());
            std::fwrite(cloud.data(), sizeof(double), cloud.size(), o);
            std::fwrite(tracker.pos(s), sizeof(double), 3, o);
            std::fwrite(tracker.quats(s), sizeof(double), 4 * (size_t)J, o);
            std::fwrite(tracker.shape(s), sizeof(double), (size_t)K, o);
        }
    }
    std::fclose(o);
    if (reps > 0 && nframes > 1) {
        std::vector<std::vector<ark::MultiFrameTracker::Frame>> steps;
        for (int t = 1; t < nframes; ++t) steps.push_back(step_frames(t));
        long n = 0, gn = 0, nsteps = 0;
        const auto t0 = std::chrono::steady_clock::now();
        for (int r = 0; r < reps; ++r)
            for (const auto& fr : steps) {
                tracker.process(fr, fitted);
                ++nsteps;
                for (int s = 0; s < S; ++s) {
                    if (!fitted[(size_t)s]) continue;
                    ++n; gn += tracker.stats[(size_t)s].gn_iterations;
                    if (posedTimed) tracker.posed(s, cloud.data());
                }
            }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        std::printf("multi_tracker_demo timing: %d streams, %ld steps, %ld frames, %.1f frames/s, %.4f ms per step, %.2f GN iterations per frame, posed %d\n",
                    S, nsteps, n, 1000.0 * (double)n / ms, ms / (double)nsteps, (double)gn / (double)n, posedTimed);
    }
    long fit = 0;
    for (const auto& st : tracker.streams) fit += st.framesFitted;
    std::printf("multi_tracker_demo: %d streams, %d steps, %ld fitted\n", S, nframes, fit);
    return 0;
}
