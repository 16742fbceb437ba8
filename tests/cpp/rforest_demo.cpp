// rforest_demo.cpp — the labelling step of the reference's tracker loop (demo.cpp:133, :196-204) with a forest of several
// trees in the tree's place, through the C++ facade (ark/RForest.h):
//   argv[1] depth.bin (int rows, cols, tl.x, tl.y, br.x, br.y; rows*cols floats), argv[2] out.bin (rows*cols label bytes after
//   predictBest + postProcess, then 2*numParts doubles com_pre), argv[3..] tree files in forest order.
#include <cstdio>
#include <string>
#include <vector>

#include "ark/RForest.h"

int main(int argc, char** argv) {
    if (argc < 4) { std::fprintf(stderr, "usage: rforest_demo depth.bin out.bin tree [tree ...]\n"); return 2; }
    ark::RForest forest(std::vector<std::string>(argv + 3, argv + argc));
    if (forest.numParts <= 0) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror("depth"); return 2; }
    int hdr[6];
    if (std::fread(hdr, sizeof(int), 6, f) != 6) return 2;
    ark::ImageF depth(hdr[0], hdr[1]);
    if (std::fread(depth.data(), sizeof(float), depth.a.size(), f) != depth.a.size()) return 2;
    std::fclose(f);
    const ark::Point topLeft(hdr[2], hdr[3]), botRight(hdr[4], hdr[5]);
    ark::MatrixNX<2> comPre;                                            // demo.cpp:148
    ark::Image8 result = forest.predictBest(depth, 8, 2, topLeft, botRight);
    forest.postProcess(result, comPre, 2, 8, topLeft, botRight);
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) { std::perror("out"); return 2; }
    std::fwrite(result.data(), 1, result.a.size(), o);
    std::fwrite(comPre.data(), sizeof(double), comPre.size(), o);
    std::fclose(o);
    size_t labelled = 0;
    for (uint8_t v : result.a) labelled += v != 255;
    std::printf("rforest_demo: %d trees, %d parts, %d nodes, %zu labelled pixels\n", forest.numTrees, forest.numParts, forest.totalNodes, labelled);
    return 0;
}
