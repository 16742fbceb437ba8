// avatar_renderer_restatement.cpp — CPU restatement of ark::AvatarRenderer's four outputs (AvatarRenderer.cpp:11-224) for the
// tests of include/avt_render.h.  Compiled at test time with g++ -ffp-contract=off.  The fills, the projection and the painter
// order are the render oracle's (oracle/render_oracle.cpp, included unchanged); this file adds what the oracle does not restate:
//   * renderLambert: face normals (b - a) x (c - a) through Eigen 3.3's normalized() (zero vector unchanged) summed into their
//     vertices in painter order, each vertex sum divided by its norm (colwise().normalize(): no zero guard), negated if z > 0,
//     the two lights in double, float * 255 and std::max(., 0.f); faces with fabs(n_z) > 1e-2 painted with the barycentric
//     row fill, the float image converted to uint8 as x86 does (truncation, NaN -> 0)
//   * renderFaces: the end-exclusive single-colour fill of every face with its painter position, background -1
//   * getProjectedJoints and getOrderedFaces
// Sums of three terms go left to right.
#include "../../oracle/render_oracle.cpp"

namespace {

void face_normal(const double* a, const double* b, const double* c, double n[3]) {
    const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    n[0] = ab[1] * ac[2] - ab[2] * ac[1];
    n[1] = ab[2] * ac[0] - ab[0] * ac[2];
    n[2] = ab[0] * ac[1] - ab[1] * ac[0];
    const double z = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
    if (z > 0.0) { const double s = std::sqrt(z); n[0] = n[0] / s; n[1] = n[1] / s; n[2] = n[2] / s; }
}

double light_dot(const double light[3], const double* p, const double* n) {
    double l[3] = {light[0] - p[0], light[1] - p[1], light[2] - p[2]};
    const double z = l[0] * l[0] + l[1] * l[1] + l[2] * l[2];
    if (z > 0.0) { const double s = std::sqrt(z); l[0] = l[0] / s; l[1] = l[1] / s; l[2] = l[2] / s; }
    return l[0] * n[0] + l[1] * n[1] + l[2] * n[2];
}

std::uint8_t to_u8(float v) { return std::isnan(v) ? 0 : (std::uint8_t)(int)v; }   // values are in [0, 255] or NaN

}  // namespace

extern "C" {

// Any output pointer may be NULL.  mesh F x 3, cloud V x 3, joints J x 3 (NULL when J = 0), vertex_part V.
// vnormal_out V x 3 and lambert_v_out V: the per-vertex normals and Lambert values of renderLambert.
int rst_render(int V, int F, int J, const double* cloud, const double* joints, const int* mesh, const int* vertex_part, float fx, float fy,
               float cx, float cy, int W, int H, int stable, float* depth_out, std::uint8_t* mask_out, std::uint8_t* lambert_out, int* faces_out,
               float* proj_out, float* jproj_out, float* keys_out, int* ordered_out, double* vnormal_out, float* lambert_v_out) {
    std::vector<P2> pr, jp;
    project_points(V, cloud, fx, fy, cx, cy, pr);
    if (J > 0 && joints) project_points(J, joints, fx, fy, cx, cy, jp);
    std::vector<std::pair<float, int>> faces;
    ordered_faces(F, mesh, cloud, faces, stable != 0);
    if (proj_out) for (int i = 0; i < V; ++i) { proj_out[2 * i] = pr[i].x; proj_out[2 * i + 1] = pr[i].y; }
    if (jproj_out) for (int i = 0; i < J; ++i) { jproj_out[2 * i] = jp[i].x; jproj_out[2 * i + 1] = jp[i].y; }
    for (int k = 0; k < F; ++k) {
        if (keys_out) keys_out[k] = faces[k].first;
        if (ordered_out) for (int c = 0; c < 3; ++c) ordered_out[3 * k + c] = mesh[3 * (size_t)faces[k].second + c];
    }
    const size_t npix = (size_t)W * H;
    if (depth_out || mask_out) {
        std::vector<float> depth(depth_out ? npix : 0, 0.f);
        std::vector<std::uint8_t> mask(mask_out ? npix : 0, 255);
        for (int k = 0; k < F; ++k) {
            const int* fc = mesh + 3 * (size_t)faces[k].second;
            const double* a = cloud + 3 * (size_t)fc[0]; const double* b = cloud + 3 * (size_t)fc[1]; const double* c = cloud + 3 * (size_t)fc[2];
            const bool eo = edge_on(a, b, c);
            if (depth_out) {
                if (eo) paint_single<float>(depth, W, H, pr, fc, 0.f);
                else { const float zv[3] = {(float)a[2], (float)b[2], (float)c[2]}; paint_bary(depth, W, H, pr, fc, zv, 255.0f); }
            }
            if (mask_out) {
                if (eo) paint_single<std::uint8_t>(mask, W, H, pr, fc, (std::uint8_t)255);
                else paint_parts(mask, W, H, pr, fc, vertex_part);
            }
        }
        if (depth_out) std::copy(depth.begin(), depth.end(), depth_out);
        if (mask_out) std::copy(mask.begin(), mask.end(), mask_out);
    }
    if (lambert_out || vnormal_out || lambert_v_out) {
        std::vector<double> vn((size_t)3 * V, 0.0);
        std::vector<char> visible((size_t)F);
        for (int k = 0; k < F; ++k) {
            const int* fc = mesh + 3 * (size_t)faces[k].second;
            double n[3];
            face_normal(cloud + 3 * (size_t)fc[0], cloud + 3 * (size_t)fc[1], cloud + 3 * (size_t)fc[2], n);
            for (int j = 0; j < 3; ++j) for (int c = 0; c < 3; ++c) vn[3 * (size_t)fc[j] + c] += n[c];
            visible[(size_t)k] = std::fabs(n[2]) > 1e-2;
        }
        std::vector<float> lam((size_t)V);
        const double main_light[3] = {0.8, 1.5, -1.2}, back_light[3] = {-0.2, -1.5, 0.4};
        for (int v = 0; v < V; ++v) {
            double* n = &vn[3 * (size_t)v];
            const double nrm = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
            n[0] = n[0] / nrm; n[1] = n[1] / nrm; n[2] = n[2] / nrm;
            if (n[2] > 0) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
            const double* p = cloud + 3 * (size_t)v;
            lam[(size_t)v] = std::max(float(light_dot(main_light, p, n) * 0.8 + light_dot(back_light, p, n) * 0.2) * 255, 0.f);
        }
        if (vnormal_out) std::copy(vn.begin(), vn.end(), vnormal_out);
        if (lambert_v_out) std::copy(lam.begin(), lam.end(), lambert_v_out);
        if (lambert_out) {
            std::vector<float> gray(npix, 0.f);
            for (int k = 0; k < F; ++k) {
                if (!visible[(size_t)k]) continue;
                const int* fc = mesh + 3 * (size_t)faces[k].second;
                const float zv[3] = {lam[(size_t)fc[0]], lam[(size_t)fc[1]], lam[(size_t)fc[2]]};
                paint_bary(gray, W, H, pr, fc, zv, 255.0f);
            }
            for (size_t i = 0; i < npix; ++i) lambert_out[i] = to_u8(gray[i]);
        }
    }
    if (faces_out) {
        std::vector<int> fimg(npix, -1);
        for (int k = 0; k < F; ++k) paint_single<int>(fimg, W, H, pr, mesh + 3 * (size_t)faces[k].second, k);
        std::copy(fimg.begin(), fimg.end(), faces_out);
    }
    return 0;
}

}  // extern "C"
