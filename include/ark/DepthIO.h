// ark/DepthIO.h — the reference's `.depth` codec: ark::util::readDepth, writeDepth and readXYZ (Util.cpp:176-247) on
// ark::ImageDepth / ark::ImageXYZ.  Header-only, no OpenCV; avatar_amd/depth.py is the Python mirror, byte for byte.
//
// The format: uint16 rows, uint16 cols, then little-endian float32 words.  A word >= 0 is a literal pixel; a word x < 0 is a
// run of (int)(-x) zero pixels, which continues across row ends.  The writer drops a trailing run and takes -0.0 for zero.
// Kept from the reference: a negative depth is written as a literal and reads back as a run; run lengths are floats, exact
// only below 2^24.  Where the reference is undefined or reads garbage: a NaN word is a literal NaN pixel; a
// run ends at the image's end at the latest (-inf and magnitudes beyond int included); a file that ends early leaves the
// remaining pixels 0; rows or cols 0 give an empty image.  Like the reference's reader (cv::Mat::zeros, :189) this one allocates the
// rows x cols image the header names before it reads the body: an all-zero image of any size is a 4-byte file, so the file's
// length bounds nothing; a caller who reads untrusted files checks the header first.  The .exr branch of readDepth needs OpenCV and is not built.
#pragma once
#include <cstdint>
#include <cstring>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <string>
#include <vector>

#include "Types.h"

namespace ark {
namespace util {

/** The image of a `.depth` file's bytes (Util.cpp:183-208) */
inline ImageDepth decodeDepth(const std::vector<unsigned char>& buf) {
    if (buf.size() < 4) return ImageDepth();
    const int rows = buf[0] | (buf[1] << 8), cols = buf[2] | (buf[3] << 8);     // little-endian uint16: hi, then wid (:185-187)
    ImageDepth m(rows, cols);
    const size_t n = (size_t)rows * cols, words = (buf.size() - 4) / 4;
    size_t i = 0;
    for (size_t k = 0; k < words && i < n; ++k) {
        const unsigned char* b = buf.data() + 4 + 4 * k;
        const std::uint32_t u = (std::uint32_t)b[0] | ((std::uint32_t)b[1] << 8) | ((std::uint32_t)b[2] << 16) | ((std::uint32_t)b[3] << 24);
        float x;
        std::memcpy(&x, &u, sizeof x);
        if (!(x < 0)) {                      // a literal: >= 0, or NaN
            m.a[i++] = x;
        } else {                             // (int)(-x) zeros, to the image's end at the most
            const double run = -(double)x, left = (double)(n - i);   // both exact in double (n < 2^32), as the Python mirror compares
            i += run >= left ? n - i : (size_t)run;
        }
    }
    return m;
}

/** The bytes util::writeDepth writes (Util.cpp:219-247) */
inline std::vector<unsigned char> encodeDepth(const ImageDepth& depth_map) {
    if (depth_map.rows < 0 || depth_map.rows > 65535 || depth_map.cols < 0 || depth_map.cols > 65535)
        throw std::invalid_argument("writeDepth: rows and cols must fit uint16");
    std::vector<unsigned char> out;
    auto put16 = [&](unsigned v) { out.push_back((unsigned char)(v & 255)); out.push_back((unsigned char)(v >> 8)); };
    auto put = [&](float v) {
        std::uint32_t u;
        std::memcpy(&u, &v, sizeof u);
        for (int s = 0; s < 32; s += 8) out.push_back((unsigned char)((u >> s) & 255));
    };
    put16((unsigned)depth_map.rows);
    put16((unsigned)depth_map.cols);
    int zrun = 0;
    for (float v : depth_map.a) {
        if (v == 0) { ++zrun; continue; }    // -0.0 too
        if (zrun >= 1) put((float)(-zrun));
        zrun = 0;
        put(v);
    }
    return out;
}

inline bool isExr(const std::string& path) { return path.size() > 4 && !path.compare(path.size() - 4, 4, ".exr"); }

/** util::readDepth (Util.cpp:176-209).  A file that cannot be opened gives an empty image (the reference reads an unset header);
 *  an .exr path throws: that branch needs OpenCV and is not built. */
inline void readDepth(const std::string& path, ImageDepth& m, bool allow_exr = true) {
    if (allow_exr && isExr(path)) throw std::runtime_error("readDepth: the .exr branch needs OpenCV and is not built: " + path);
    std::ifstream ifs(path, std::ios::binary | std::ios::in);
    std::vector<unsigned char> buf((std::istreambuf_iterator<char>(ifs)), std::istreambuf_iterator<char>());
    m = decodeDepth(buf);
}

/** util::writeDepth (Util.cpp:219-247); like the reference, silent when the file cannot be opened */
inline void writeDepth(const std::string& image_path, const ImageDepth& depth_map) {
    const std::vector<unsigned char> out = encodeDepth(depth_map);
    std::ofstream ofsd(image_path, std::ios::binary | std::ios::out);
    if (ofsd) ofsd.write((const char*)out.data(), (std::streamsize)out.size());
}

/** util::readXYZ (Util.cpp:211-217): readDepth, then depthToXYZ unless the image is empty */
inline void readXYZ(const std::string& path, ImageXYZ& m, const CameraIntrin& intrin, bool allow_exr = true) {
    ImageDepth d;
    readDepth(path, d, allow_exr);
    m = d.empty() ? ImageXYZ(d.rows, d.cols) : intrin.depthToXYZ(d);
}

}  // namespace util
}  // namespace ark
