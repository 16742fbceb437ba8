"""The z-buffer frame generator (avt_synth_render_frames: k_raster, k_raster_label, k_raster_scan, k_raster_emit of
avatar_amd/csrc/avt_render.hip; host twin avatar_amd/csrc/synth_render.cpp) restated in numpy from the header comment of
synth_render.cpp.  A helper module of the tests, not a test file.

The operation, per frame:
  * every vertex p projects to (float)(p.x fx / p.z + cx), (float)(-p.y fy / p.z + cy), the quotient and sum in double;
  * a face is dropped when its normal (b - a) x (c - a) has length 0 or |n_z| / |n| < 0.1 (edge-on), when a vertex has z <= 0, or
    when its three projections are collinear (the float denominator of the barycentric weights is 0);
  * it covers the integer pixel centres (col, row) of its bounding box - floor of the smallest, ceil of the largest projected
    coordinate, each clamped in float to the image (min bounds to [0, size], max bounds to [-1, size - 1]) - whose three float
    barycentric weights are all >= 0 (a centre on an edge is inside), with the screen-space linear depth z = w1 az + w2 bz + w3 cz,
    and only where z > 0;
  * a pixel shows the covering face with the smallest (depth bits, face id);
  * its label is the part of the winning face's nearest projected vertex by float squared distance:
    (da < db && da < dc) ? a : (db < dc ? b : c);
  * the foreground pixels are back-projected in row-major order with float arithmetic, X = (col - cx) z / fx, Y = (row - cy) z / fy,
    and returned as doubles (X, -Y, z).

Every float expression is written in the order of the source with explicit np.float32 / np.float64 operands (numpy neither
contracts nor reassociates); visibility is the minimum of a 64-bit key, not the host's in-order strict '<'."""
from __future__ import annotations

import numpy as np

F32 = np.float32
BACKGROUND = np.uint64(0xFFFFFFFFFFFFFFFF)


def project(cloud, k):
    """(px, py) float32 of every vertex; vertices at z == 0 give inf / nan like the sources (never used: z <= 0 drops the face)."""
    c = np.asarray(cloud, np.float64)
    fx, fy, cx, cy = (np.float64(k[n]) for n in ("fx", "fy", "cx", "cy"))
    with np.errstate(all="ignore"):
        px = (c[:, 0] * fx / c[:, 2] + cx).astype(F32)
        py = (-c[:, 1] * fy / c[:, 2] + cy).astype(F32)
    return px, py


def face_is_drawn(a, b, c):
    """the two rejection rules that use the camera-space vertices (float64 scalars in the written order)"""
    ab = [np.float64(b[i]) - np.float64(a[i]) for i in range(3)]
    ac = [np.float64(c[i]) - np.float64(a[i]) for i in range(3)]
    with np.errstate(all="ignore"):
        n0 = ab[1] * ac[2] - ab[2] * ac[1]
        n1 = ab[2] * ac[0] - ab[0] * ac[2]
        n2 = ab[0] * ac[1] - ab[1] * ac[0]
        nn = np.sqrt(n0 * n0 + n1 * n1 + n2 * n2)
        if not (nn > 0.0) or np.abs(n2 / nn) < 0.1:
            return False
    return not (a[2] <= 0.0 or b[2] <= 0.0 or c[2] <= 0.0)


def clamped_box(lo, hi, size):
    """[first, last] pixel index along one axis from the smallest / largest projected coordinate (float32), clamped in float"""
    first = min(max(np.floor(lo), F32(0.0)), F32(size))
    last = min(max(np.ceil(hi), F32(-1.0)), F32(size - 1))
    return int(first), int(last)


def render(cloud, mesh, vertex_part, k, width, height):
    """depth (H,W) float32 (inf = background), face (H,W) int32 (-1 = background), label (H,W) int32 (-1 = background),
    data (N,3) float64, labels (N,) int32 in row-major pixel order."""
    cloud = np.asarray(cloud, np.float64)
    mesh = np.asarray(mesh, np.int64).reshape(-1, 3)
    vp = np.asarray(vertex_part, np.int32)
    px, py = project(cloud, k)
    key = np.full((height, width), BACKGROUND, np.uint64)
    one = F32(1.0)
    with np.errstate(all="ignore"):
        for f, (ia, ib, ic) in enumerate(mesh):
            if not face_is_drawn(cloud[ia], cloud[ib], cloud[ic]):
                continue
            ax, ay, bx, by, cxx, cyy = px[ia], py[ia], px[ib], py[ib], px[ic], py[ic]
            denom = (by - cyy) * (ax - cxx) + (cxx - bx) * (ay - cyy)
            if denom == F32(0.0):
                continue
            inv = one / denom
            x0, x1 = clamped_box(min(ax, min(bx, cxx)), max(ax, max(bx, cxx)), width)
            y0, y1 = clamped_box(min(ay, min(by, cyy)), max(ay, max(by, cyy)), height)
            if x1 < x0 or y1 < y0:
                continue
            col = np.arange(x0, x1 + 1).astype(F32)[None, :]
            row = np.arange(y0, y1 + 1).astype(F32)[:, None]
            w1 = ((by - cyy) * (col - cxx) + (cxx - bx) * (row - cyy)) * inv
            w2 = ((cyy - ay) * (col - cxx) + (ax - cxx) * (row - cyy)) * inv
            w3 = one - w1 - w2
            az, bz, cz = F32(cloud[ia, 2]), F32(cloud[ib, 2]), F32(cloud[ic, 2])
            z = w1 * az + w2 * bz + w3 * cz
            assert w1.dtype == w2.dtype == w3.dtype == z.dtype == F32
            inside = ~((w1 < 0) | (w2 < 0) | (w3 < 0)) & (z > 0)
            fkey = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(f)
            sub = key[y0:y1 + 1, x0:x1 + 1]
            sub[inside] = np.minimum(sub[inside], fkey[inside])
        fg = key != BACKGROUND
        depth = np.where(fg, (key >> np.uint64(32)).astype(np.uint32).view(F32), F32(np.inf)).astype(F32)
        face = np.where(fg, (key & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
        label = np.full((height, width), -1, np.int32)
        rr, cc = np.nonzero(fg)
        if len(rr):
            wf = mesh[face[rr, cc]]
            r32, c32 = rr.astype(F32), cc.astype(F32)
            d = []
            for s in range(3):
                vx, vy = px[wf[:, s]], py[wf[:, s]]
                d.append((vx - c32) * (vx - c32) + (vy - r32) * (vy - r32))
            da, db, dc = d
            pick = np.where((da < db) & (da < dc), 0, np.where(db < dc, 1, 2))
            label[rr, cc] = vp[wf[np.arange(len(rr)), pick]]
        data, labels = backproject(depth, label, k)
    return depth, face, label, data, labels


def backproject(depth, label, k):
    """CameraIntrin::to3D in float, y negated, row-major order of the pixels with a label"""
    ffx, ffy, fcx, fcy = (F32(np.float64(k[n])) for n in ("fx", "fy", "cx", "cy"))
    rr, cc = np.nonzero(label >= 0)
    z = depth[rr, cc].astype(F32)
    X = (cc.astype(F32) - fcx) * z / ffx
    Y = (rr.astype(F32) - fcy) * z / ffy
    assert X.dtype == Y.dtype == F32
    data = np.stack([X.astype(np.float64), -Y.astype(np.float64), z.astype(np.float64)], 1).reshape(-1, 3)
    return data, label[rr, cc].astype(np.int32)
