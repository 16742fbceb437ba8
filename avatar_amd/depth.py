"""Depth images in: the host side of the reference's recorded-data path (demo.cpp:126,166).

`CameraIntrin` with `to3D` / `to2D` (Calibration.cpp:68-80), `depth_to_xyz` (`CameraIntrin::depthToXYZ`, :82-95) and the
`.depth` codec `read_depth` / `write_depth` / `read_xyz` (`util::readDepth`, `writeDepth`, `readXYZ`, Util.cpp:176-247).
All of it is float32 in the reference's expression order: the int column converted to float, minus cx, times z, divided
by fx; no reciprocal, no fused operation, no double.  include/ark/Types.h and include/ark/DepthIO.h are the C++ mirror;
avatar_amd/csrc/avt_bgsub.hip's k_bgs_backproject computes the same on the device.

The `.depth` format: uint16 rows, uint16 cols, then little-endian float32 words; a word >= 0 is a literal pixel, a word
x < 0 a run of (int)(-x) zero pixels that continues across row ends.  The writer drops a trailing run and takes -0.0 for
zero.  Where the reference is undefined: a NaN word is a literal NaN pixel, a run ends at the image's
end at the latest, a file that ends early leaves the remaining pixels 0, rows or cols 0 give an empty image."""
from __future__ import annotations

import numpy as np

F = np.float32


class CameraIntrin:
    """fx, fy, cx, cy as float32 (Calibration.h:11-77; the defaults are the reference's).  The distortion terms k[], p[] are
    carried by the reference's struct and ignored by these three members there too."""

    def __init__(self, fx=606.438, fy=606.351, cx=637.294, cy=366.992):
        self.fx, self.fy, self.cx, self.cy = F(fx), F(fy), F(cx), F(cy)

    @classmethod
    def of(cls, intrin):
        """A CameraIntrin, or (fx, fy, cx, cy)."""
        return intrin if isinstance(intrin, cls) else cls(*np.asarray(intrin, F).reshape(4))

    def as_array(self):
        return np.array([self.fx, self.fy, self.cx, self.cy], F)

    def to3D(self, point, depth):
        """Calibration.cpp:68-74: pixel (x, y) at `depth` to camera coordinates, (3,) float32."""
        z = F(depth)
        with np.errstate(all="ignore"):
            return np.array([(F(point[0]) - self.cx) * z / self.fx, (F(point[1]) - self.cy) * z / self.fy, z], F)

    def to2D(self, point):
        """Calibration.cpp:76-80: camera coordinates to the pixel (x, y), (2,) float32."""
        p = np.asarray(point, F)
        with np.errstate(all="ignore"):
            return np.array([p[0] * self.fx / p[2] + self.cx, p[1] * self.fy / p[2] + self.cy], F)

    def depthToXYZ(self, depth):
        return depth_to_xyz(depth, self)


def intrin_array(intrin, n):
    """One camera (a CameraIntrin or fx, fy, cx, cy) for all n images, or (n, 4): the (n, 4) float32 array of the C ABI."""
    a = intrin.as_array() if isinstance(intrin, CameraIntrin) else np.asarray(intrin, F)
    if a.shape == (4,):
        a = np.tile(a, (n, 1))
    if a.shape != (n, 4):
        raise ValueError(f"intrinsics must be one camera (fx, fy, cx, cy) or ({n}, 4), not {a.shape}")
    return np.ascontiguousarray(a, F)


def depth_to_xyz(depth, intrin):
    """`CameraIntrin::depthToXYZ` (Calibration.cpp:82-95): (rows, cols) float32 depth to the (rows, cols, 3) XYZ map."""
    k = CameraIntrin.of(intrin)
    z = np.ascontiguousarray(depth, F)
    if z.ndim != 2:
        raise ValueError("depth_to_xyz: depth must be (rows, cols)")
    rows, cols = z.shape
    xyz = np.empty((rows, cols, 3), F)
    with np.errstate(all="ignore"):          # 0 * inf, inf / x and the like give what IEEE gives, as in the reference
        xyz[:, :, 0] = (np.arange(cols, dtype=np.int32).astype(F)[None, :] - k.cx) * z / k.fx
        xyz[:, :, 1] = (np.arange(rows, dtype=np.int32).astype(F)[:, None] - k.cy) * z / k.fy
    xyz[:, :, 2] = z
    return xyz


def decode_depth(buf):
    """The image of a `.depth` file's bytes (util::readDepth, Util.cpp:183-208)."""
    if len(buf) < 4:
        return np.zeros((0, 0), F)
    rows, cols = (int(v) for v in np.frombuffer(buf, "<u2", 2))
    n = rows * cols
    out = np.zeros(n, F)
    words = np.frombuffer(buf, "<f4", (len(buf) - 4) // 4, 4)
    i = 0
    for w in words:
        if i >= n:
            break
        if not w < 0:                        # a literal: >= 0, or NaN
            out[i] = w
            i += 1
        else:                                # (int)(-x) zeros, to the image's end at the most (-inf, magnitudes beyond int)
            i += int(min(np.float64(-w), n - i))
    return out.reshape(rows, cols)


def encode_depth(depth):
    """The bytes util::writeDepth (Util.cpp:219-247) writes for a (rows, cols) float32 image, rows and cols < 65536."""
    z = np.ascontiguousarray(depth, F)
    if z.ndim != 2 or z.shape[0] > 65535 or z.shape[1] > 65535:
        raise ValueError("encode_depth: depth must be (rows, cols) with rows, cols < 65536")
    flat = z.ravel()
    words, run = [], 0
    for v in flat:
        if v == 0:                           # -0.0 too
            run += 1
            continue
        if run >= 1:
            words.append(F(-run))
        run = 0
        words.append(v)
    return np.array(z.shape, "<u2").tobytes() + np.array(words, "<f4").tobytes()


def _no_exr(path, what):
    if str(path).endswith(".exr"):
        raise ValueError(f"{what}: the .exr branch of util::readDepth needs OpenCV and is not built: {path}")


def read_depth(path):
    _no_exr(path, "read_depth")
    with open(path, "rb") as f:
        return decode_depth(f.read())


def write_depth(path, depth):
    with open(path, "wb") as f:
        f.write(encode_depth(depth))


def read_xyz(path, intrin):
    """util::readXYZ (Util.cpp:211-217): read_depth, then depth_to_xyz unless the image is empty."""
    d = read_depth(path)
    return depth_to_xyz(d, intrin) if d.size else np.zeros(d.shape + (3,), F)
