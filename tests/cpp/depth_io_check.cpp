// depth_io_check.cpp — CPU-only check of include/ark/DepthIO.h and ark::CameraIntrin (tests/test_depth_in_cpu.py):
//   depth_io_check codec in.depth out.depth out.raw     readDepth, then writeDepth of the image and a raw dump of it
//   depth_io_check xyz in.raw fx fy cx cy out.raw       depthToXYZ of a raw image, dumped raw
//   depth_io_check exr path                             readDepth must refuse the .exr branch: exit status 4
// A raw file is int32 rows, cols, then the float32 values.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ark/DepthIO.h"
#include "ark/Types.h"

static bool dump(const char* path, int rows, int cols, const std::vector<float>& a) {
    FILE* o = std::fopen(path, "wb");
    if (!o) return false;
    const int h[2] = {rows, cols};
    std::fwrite(h, sizeof(int), 2, o);
    if (!a.empty()) std::fwrite(a.data(), sizeof(float), a.size(), o);
    return std::fclose(o) == 0;
}

int main(int argc, char** argv) {
    if (argc == 5 && !std::strcmp(argv[1], "codec")) {
        ark::ImageDepth m;
        ark::util::readDepth(argv[2], m);
        ark::util::writeDepth(argv[3], m);
        return dump(argv[4], m.rows, m.cols, m.a) ? 0 : 2;
    }
    if (argc == 8 && !std::strcmp(argv[1], "xyz")) {
        FILE* f = std::fopen(argv[2], "rb");
        int h[2];
        if (!f || std::fread(h, sizeof(int), 2, f) != 2) return 2;
        ark::ImageDepth d(h[0], h[1]);
        if (std::fread(d.data(), sizeof(float), d.a.size(), f) != d.a.size()) return 2;
        std::fclose(f);
        ark::CameraIntrin k;
        k.fx = std::strtof(argv[3], nullptr); k.fy = std::strtof(argv[4], nullptr);
        k.cx = std::strtof(argv[5], nullptr); k.cy = std::strtof(argv[6], nullptr);
        const ark::ImageXYZ xyz = k.depthToXYZ(d);
        return dump(argv[7], xyz.rows, xyz.cols, xyz.a) ? 0 : 2;
    }
    if (argc == 3 && !std::strcmp(argv[1], "exr")) {
        ark::ImageDepth m;
        try {
            ark::util::readDepth(argv[2], m);
        } catch (const std::exception& e) {
            std::fprintf(stderr, "depth_io_check: %s\n", e.what());
            return 4;
        }
        return 0;
    }
    std::fprintf(stderr, "usage: depth_io_check codec in.depth out.depth out.raw | xyz in.raw fx fy cx cy out.raw | exr path\n");
    return 2;
}
