// bgsub_demo.cpp — the background subtraction step of the reference's tracker loop through the C++ facade
// (demo.cpp:179-192, live-demo.cpp:317-332):
//   argv[1] in.bin: int rows, cols, n_frames; float nn_rel, neighb_rel; the background (rows*cols*3 floats), then
//           n_frames XYZ maps, run one after another through the same ark::BGSubtractor
//   argv[2] out.bin: per frame rows*cols mask bytes, int tl.x tl.y br.x br.y fg_count n_comps, n_comps x {size, id},
//           rows*cols floats of masked depth.
#include <array>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ark/BGSubtractor.h"

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: bgsub_demo in.bin out.bin\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror("in"); return 2; }
    int hdr[3];
    float rel[2];
    if (std::fread(hdr, sizeof(int), 3, f) != 3 || std::fread(rel, sizeof(float), 2, f) != 2) return 2;
    ark::ImageXYZ bgimg(hdr[0], hdr[1]);
    if (std::fread(bgimg.data(), sizeof(float), bgimg.a.size(), f) != bgimg.a.size()) return 2;
    ark::BGSubtractor bgsub(bgimg);
    bgsub.nnDistThreshRel = rel[0];
    bgsub.neighbThreshRel = rel[1];
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) { std::perror("out"); return 2; }
    ark::ImageXYZ image(hdr[0], hdr[1]);
    for (int i = 0; i < hdr[2]; ++i) {
        if (std::fread(image.data(), sizeof(float), image.a.size(), f) != image.a.size()) return 2;
        std::vector<std::array<int, 2>> compsBySize;
        ark::Image8 sub = bgsub.run(image, &compsBySize);
        const int rec[6] = {bgsub.topLeft.x, bgsub.topLeft.y, bgsub.botRight.x, bgsub.botRight.y, bgsub.foregroundCount(), (int)compsBySize.size()};
        std::fwrite(sub.data(), 1, sub.a.size(), o);
        std::fwrite(rec, sizeof(int), 6, o);
        for (const auto& c : compsBySize) std::fwrite(c.data(), sizeof(int), 2, o);
        std::fwrite(bgsub.maskedDepth().data(), sizeof(float), bgsub.maskedDepth().a.size(), o);
        std::printf("bgsub_demo: frame %d box (%d,%d)-(%d,%d), %zu components, %d foreground pixels\n", i, rec[0], rec[1], rec[2], rec[3],
                    compsBySize.size(), rec[4]);
    }
    std::fclose(f);
    std::fclose(o);
    return 0;
}
