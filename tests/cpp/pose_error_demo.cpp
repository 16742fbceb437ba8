// pose_error_demo — ark::PoseErrorResult::derive() for tests/test_pose_error_cpu.py (no GPU):
//   pose_error_demo derive in.bin out.bin
//   pose_error_demo score in.bin out.bin      (GPU: ark::PoseError on uploaded pairs, tests/test_gpu_pose_error.py)
// in:  int32 V, J, P; AVT_POSEERR_COLS doubles (a summary row); P doubles PART_SUM; P int32 part sizes
// out: pve, pveRms, pveMax, paPve, paPveScale, mpjpe, mpjpeMax, mpjpeRoot, paMpjpe, paMpjpeScale, then P doubles pvePart
// score in:  int32 V, J, P, n; V int32 vertex_part; doubles: n x 3V and n x 3J of the estimate, then of the truth
// score out: per pair AVT_POSEERR_COLS doubles, J raw and J aligned joint errors, P part sums and P part maxima, then as doubles
//            the two argmax and the status; then derive().pve
#include <cstdio>
#include <cstring>
#include <vector>

#include "ark/PoseError.h"

static int derive_mode(const char* in, const char* out) {
    FILE* f = std::fopen(in, "rb");
    if (!f) { std::fprintf(stderr, "cannot read %s\n", in); return 1; }
    int dims[3];
    ark::PoseErrorResult r;
    bool ok = std::fread(dims, sizeof(int), 3, f) == 3 && dims[2] >= 0;
    if (ok) {
        r.V = dims[0]; r.J = dims[1]; r.numParts = dims[2];
        r.partSum.resize((size_t)r.numParts);
        r.partSize.resize((size_t)r.numParts);
        ok = std::fread(r.summary, sizeof(double), AVT_POSEERR_COLS, f) == AVT_POSEERR_COLS &&
             std::fread(r.partSum.data(), sizeof(double), (size_t)r.numParts, f) == (size_t)r.numParts &&
             std::fread(r.partSize.data(), sizeof(int), (size_t)r.numParts, f) == (size_t)r.numParts;
    }
    std::fclose(f);
    if (!ok) { std::fprintf(stderr, "short input %s\n", in); return 1; }
    const ark::PoseErrorFigures g = r.derive();
    std::vector<double> v = {g.pve, g.pveRms, g.pveMax, g.paPve, g.paPveScale, g.mpjpe, g.mpjpeMax, g.mpjpeRoot, g.paMpjpe, g.paMpjpeScale};
    v.insert(v.end(), g.pvePart.begin(), g.pvePart.end());
    FILE* o = std::fopen(out, "wb");
    if (!o || std::fwrite(v.data(), sizeof(double), v.size(), o) != v.size()) { std::fprintf(stderr, "cannot write %s\n", out); return 1; }
    std::fclose(o);
    return 0;
}

static int score_mode(const char* in, const char* out) {
    FILE* f = std::fopen(in, "rb");
    if (!f) { std::fprintf(stderr, "cannot read %s\n", in); return 1; }
    int d[4];
    if (std::fread(d, sizeof(int), 4, f) != 4) { std::fprintf(stderr, "short input %s\n", in); return 1; }
    const size_t V = (size_t)d[0], J = (size_t)d[1], n = (size_t)d[3];
    std::vector<int> vp(V);
    std::vector<double> ec(n * 3 * V), ej(n * 3 * J), tc(n * 3 * V), tj(n * 3 * J);
    const bool ok = std::fread(vp.data(), sizeof(int), V, f) == V && std::fread(ec.data(), sizeof(double), ec.size(), f) == ec.size() &&
                    std::fread(ej.data(), sizeof(double), ej.size(), f) == ej.size() && std::fread(tc.data(), sizeof(double), tc.size(), f) == tc.size() &&
                    std::fread(tj.data(), sizeof(double), tj.size(), f) == tj.size();
    std::fclose(f);
    if (!ok) { std::fprintf(stderr, "short input %s\n", in); return 1; }
    ark::PoseError pe(d[0], d[1], d[2], vp, (int)n);
    pe.upload(AVT_POSEERR_ESTIMATE, (int)n, ec.data(), ej.data());
    pe.upload(AVT_POSEERR_TRUTH, (int)n, tc.data(), tj.data());
    pe.run();
    std::vector<double> v;
    for (const ark::PoseErrorResult& r : pe.get()) {
        v.insert(v.end(), r.summary, r.summary + AVT_POSEERR_COLS);
        v.insert(v.end(), r.jointErr.begin(), r.jointErr.end());
        v.insert(v.end(), r.jointErrAligned.begin(), r.jointErrAligned.end());
        v.insert(v.end(), r.partSum.begin(), r.partSum.end());
        v.insert(v.end(), r.partMax.begin(), r.partMax.end());
        v.push_back((double)r.vArgmax); v.push_back((double)r.jArgmax); v.push_back((double)r.status);
        v.push_back(r.derive().pve);
    }
    FILE* o = std::fopen(out, "wb");
    if (!o || std::fwrite(v.data(), sizeof(double), v.size(), o) != v.size()) { std::fprintf(stderr, "cannot write %s\n", out); return 1; }
    std::fclose(o);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && !std::strcmp(argv[1], "derive")) return derive_mode(argv[2], argv[3]);
    if (argc == 4 && !std::strcmp(argv[1], "score")) return score_mode(argv[2], argv[3]);
    std::fprintf(stderr, "usage: pose_error_demo derive in out | score in out\n");
    return 2;
}
