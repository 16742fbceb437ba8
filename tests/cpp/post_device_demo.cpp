// post_device_demo — ark::RTree / ark::RForest postProcessResident, comPre and setComPre (include/ark/RTree.h, RForest.h) on a
// batch of label images: tests/test_gpu_post_device.py compares the labels and memories this writes with the restatement.
//   post_device_demo <tree file> <input> <output>
// input: int32 n rows cols interval, float64 weight, n x 4 int32 boxes, num_parts x 2 float64 memory of slot 1, n x rows x cols
// label bytes.  output, for the tree and then for a forest of two such trees: the labels, then n x num_parts x 2 float64.
#include <array>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ark/BGSubtractor.h"
#include "ark/RForest.h"
#include "ark/RTree.h"

template <class F>
static void run(F& f, int n, int interval, double weight, const std::vector<std::array<int, 4>>& boxes, const ark::MatrixNX<2>& mem,
                const std::vector<ark::Image8>& imgs, FILE* out) {
    for (int i = 0; i < n; ++i) f.setComPre(i, i == 1 ? mem : ark::MatrixNX<2>());
    f.uploadLabels(imgs);
    const std::vector<ark::Image8> got = f.postProcessResident(interval, boxes, weight);
    for (const ark::Image8& im : got) fwrite(im.data(), 1, im.a.size(), out);
    for (int i = 0; i < n; ++i) {
        const ark::MatrixNX<2> com = f.comPre(i);
        if ((int)com.cols() != f.numParts) { fprintf(stderr, "slot %d is not sized after the run\n", i); std::exit(1); }
        fwrite(com.data(), sizeof(double), com.size(), out);
    }
}

int main(int argc, char** argv) {
    if (argc != 4) { fprintf(stderr, "usage: post_device_demo <tree> <in> <out>\n"); return 2; }
    ark::RTree tree(argv[1]), second(argv[1]);
    FILE* in = fopen(argv[2], "rb");
    if (!in || tree.numParts <= 0) { fprintf(stderr, "cannot read the inputs\n"); return 1; }
    int hdr[4];
    double weight = 0;
    if (fread(hdr, sizeof(int), 4, in) != 4 || fread(&weight, sizeof(double), 1, in) != 1) return 1;
    const int n = hdr[0], rows = hdr[1], cols = hdr[2], interval = hdr[3];
    std::vector<std::array<int, 4>> boxes((size_t)n);
    for (auto& b : boxes) if (fread(b.data(), sizeof(int), 4, in) != 4) return 1;
    ark::MatrixNX<2> mem;
    mem.resize(2, tree.numParts);
    if (fread(mem.data(), sizeof(double), mem.size(), in) != mem.size()) return 1;
    std::vector<ark::Image8> imgs((size_t)n, ark::Image8(rows, cols));
    for (ark::Image8& im : imgs) if (fread(im.data(), 1, im.a.size(), in) != im.a.size()) return 1;
    fclose(in);
    FILE* out = fopen(argv[3], "wb");
    if (!out) return 1;
    run(tree, n, interval, weight, boxes, mem, imgs, out);
    ark::RForest forest(std::vector<ark::RTree*>{&tree, &second});
    run(forest, n, interval, weight, boxes, mem, imgs, out);
    fclose(out);
    printf("post_device_demo: %d images of %d x %d at interval %d\n", n, cols, rows, interval);
    return 0;
}
