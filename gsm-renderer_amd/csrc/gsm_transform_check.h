// gsm_transform_check.h -- the host side of gsm_global_transform: gsm_global_transform_from_pose, which
// derives the descriptor of a pose in double, and the entry's checks.  Plain C++17 over include/gsm_renderer.h alone:
// no HIP, so a stand-alone CPU program (tests/host/transform_check_test.cpp) runs all of it without a device.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/gsm_renderer.h"
#include "gsm_extract_check.h"

namespace gsm {

// The renderer's SH basis of bands 1..3 at d (sh_color in gsm_device.h, the same signs and constants; index 0 is band
// 1's first function).  Every function is a homogeneous polynomial of its band's degree, so d need not be unit.
inline void transform_sh_basis(const double d[3], double b[15]) {
    const double C1 = 0.4886025119029199;
    const double C2[5] = {1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792,
                          0.5462742152960396};
    const double C3[7] = {-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154,
                          -0.4570457994644658, 1.445305721320277, -0.5900435899266435};
    const double x = d[0], y = d[1], z = d[2];
    const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
    b[0] = -C1 * y;
    b[1] = C1 * z;
    b[2] = -C1 * x;
    b[3] = C2[0] * xy;
    b[4] = C2[1] * yz;
    b[5] = C2[2] * (2.0 * zz - xx - yy);
    b[6] = C2[3] * xz;
    b[7] = C2[4] * (xx - yy);
    b[8] = C3[0] * y * (3.0 * xx - yy);
    b[9] = C3[1] * xy * z;
    b[10] = C3[2] * y * (4.0 * zz - xx - yy);
    b[11] = C3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy);
    b[12] = C3[4] * x * (4.0 * zz - xx - yy);
    b[13] = C3[5] * z * (xx - yy);
    b[14] = C3[6] * x * (xx - 3.0 * yy);
}

// D_l of the rotation R (row-major), N = 2l + 1, first = the band's first index in transform_sh_basis.
// The band is closed under rotation: b(R^T d) = M b(d) for one N x N matrix M and every d, and then
// sum_k c_k b_k(R^T d) = sum_k (M^T c)_k b_k(d), so D = M^T.  With the N fixed directions d_j below and the rows
// b(d_j)^T stacked in B, and b(R^T d_j)^T in B', B D = B'.  What is solved is B (D - I) = B' - B, by Gaussian
// elimination with partial pivoting: one pass, no iteration, no tolerance, and the identity rotation has the right
// side exactly zero, so that its D is exactly the identity.  The directions are fixed, one set per band, found by a
// search for a small condition number of B: 1.03, 1.78 and 2.29 for bands 1, 2 and 3.
template <int N> struct TransformDirs;
template <> struct TransformDirs<3> {
    static const double* at(int j) {
        static const double d[3][3] = {{-0.094, 0.453, 0.886}, {0.622, 0.711, -0.327}, {-0.785, 0.519, -0.339}};
        return d[j];
    }
};
template <> struct TransformDirs<5> {
    static const double* at(int j) {
        static const double d[5][3] = {{-0.781, -0.598, -0.179}, {-0.734, 0.399, 0.549}, {-0.896, 0.38, -0.23},
                                       {-0.285, -0.42, -0.862},  {0.16, -0.927, -0.34}};
        return d[j];
    }
};
template <> struct TransformDirs<7> {
    static const double* at(int j) {
        static const double d[7][3] = {{0.604, 0.78, -0.165},  {-0.934, -0.013, -0.358}, {0.526, 0.025, 0.85},
                                       {0.593, -0.712, -0.375}, {-0.158, 0.984, -0.083},  {-0.184, 0.194, 0.964},
                                       {-0.769, 0.511, -0.384}};
        return d[j];
    }
};
template <int N>
inline void transform_band_matrix(const double R[9], int first, double D[N * N]) {
    double A[N][2 * N];  // [B | B' - B]
    for (int j = 0; j < N; ++j) {
        const double* d = TransformDirs<N>::at(j);
        double rd[3], b[15], br[15];
        for (int c = 0; c < 3; ++c) rd[c] = (R[0 * 3 + c] * d[0] + R[1 * 3 + c] * d[1]) + R[2 * 3 + c] * d[2];  // R^T d
        transform_sh_basis(d, b);
        transform_sh_basis(rd, br);
        for (int k = 0; k < N; ++k) {
            A[j][k] = b[first + k];
            A[j][N + k] = br[first + k] - b[first + k];
        }
    }
    for (int p = 0; p < N; ++p) {
        int best = p;
        for (int r = p + 1; r < N; ++r)
            if (std::fabs(A[r][p]) > std::fabs(A[best][p])) best = r;
        if (best != p)
            for (int c = 0; c < 2 * N; ++c) {
                const double t = A[p][c];
                A[p][c] = A[best][c];
                A[best][c] = t;
            }
        for (int r = 0; r < N; ++r) {
            if (r == p) continue;
            const double f = A[r][p] / A[p][p];
            if (f == 0.0) continue;
            for (int c = p; c < 2 * N; ++c) A[r][c] -= f * A[p][c];
        }
    }
    for (int i = 0; i < N; ++i)
        for (int k = 0; k < N; ++k) D[i * N + k] = (i == k ? 1.0 : 0.0) + A[i][N + k] / A[i][i];
}

// gsm_global_transform_from_pose
inline gsm_status transform_from_pose(const float* rotation, float scale, const float* translation,
                                      gsm_global_transform_desc* out) {
    if (!rotation || !translation || !out) return GSM_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(rotation[i])) return GSM_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(translation[i])) return GSM_ERR_INVALID_ARGUMENT;
    if (!std::isfinite(scale) || !(scale > 0.0f)) return GSM_ERR_INVALID_ARGUMENT;
    double R[9];
    for (int i = 0; i < 9; ++i) R[i] = (double)rotation[i];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            const double v = (R[r * 3] * R[c * 3] + R[r * 3 + 1] * R[c * 3 + 1]) + R[r * 3 + 2] * R[c * 3 + 2];
            if (!(std::fabs(v - (r == c ? 1.0 : 0.0)) <= 1e-4)) return GSM_ERR_INVALID_ARGUMENT;
        }
    const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) +
                       R[2] * (R[3] * R[7] - R[4] * R[6]);
    if (det < 0.0) return GSM_ERR_INVALID_ARGUMENT;
    // Nine floats are not exactly orthonormal, and what a quaternion or a band matrix of such an R is depends on the
    // method.  So R becomes the rotation nearest to it, the orthogonal factor of its polar decomposition, which is
    // unique: three Newton steps R <- (R + R^-T) / 2 (the error squares each step: 1e-4, 1e-8, 1e-16), a fixed
    // number, no tolerance.  An R that is orthonormal already (the identity, a quarter turn) is its own fixed point,
    // bit for bit.
    for (int step = 0; step < 3; ++step) {
        const double* r0 = R;
        const double* r1 = R + 3;
        const double* r2 = R + 6;
        const double C[9] = {r1[1] * r2[2] - r1[2] * r2[1], r1[2] * r2[0] - r1[0] * r2[2], r1[0] * r2[1] - r1[1] * r2[0],
                             r2[1] * r0[2] - r2[2] * r0[1], r2[2] * r0[0] - r2[0] * r0[2], r2[0] * r0[1] - r2[1] * r0[0],
                             r0[1] * r1[2] - r0[2] * r1[1], r0[2] * r1[0] - r0[0] * r1[2], r0[0] * r1[1] - r0[1] * r1[0]};
        const double d = (r0[0] * C[0] + r0[1] * C[1]) + r0[2] * C[2];
        for (int i = 0; i < 9; ++i) R[i] = 0.5 * (R[i] + C[i] / d);  // (C / d is R^-T)
    }
    const double s = (double)scale;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) out->matrix[r * 4 + c] = (float)(s * R[r * 3 + c]);
        out->matrix[r * 4 + 3] = translation[r];
    }
    // the quaternion from the largest of the four squared components (Shepperd), normalised, w >= 0
    double q[4];  // x, y, z, w
    const double tr = R[0] + R[4] + R[8];
    if (tr >= R[0] && tr >= R[4] && tr >= R[8]) {
        q[3] = 1.0 + tr;
        q[0] = R[7] - R[5];
        q[1] = R[2] - R[6];
        q[2] = R[3] - R[1];
    } else if (R[0] >= R[4] && R[0] >= R[8]) {
        q[0] = 1.0 + R[0] - R[4] - R[8];
        q[1] = R[1] + R[3];
        q[2] = R[2] + R[6];
        q[3] = R[7] - R[5];
    } else if (R[4] >= R[8]) {
        q[0] = R[1] + R[3];
        q[1] = 1.0 - R[0] + R[4] - R[8];
        q[2] = R[5] + R[7];
        q[3] = R[2] - R[6];
    } else {
        q[0] = R[2] + R[6];
        q[1] = R[5] + R[7];
        q[2] = 1.0 - R[0] - R[4] + R[8];
        q[3] = R[3] - R[1];
    }
    const double n = std::sqrt((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]));
    const double sign = q[3] < 0.0 ? -1.0 : 1.0;
    for (int i = 0; i < 4; ++i) out->quaternion[i] = (float)(sign * q[i] / n);
    out->scale = scale;
    double D1[9], D2[25], D3[49];
    transform_band_matrix<3>(R, 0, D1);
    transform_band_matrix<5>(R, 3, D2);
    transform_band_matrix<7>(R, 8, D3);
    for (int i = 0; i < 9; ++i) out->sh1[i] = (float)D1[i];
    for (int i = 0; i < 25; ++i) out->sh2[i] = (float)D2[i];
    for (int i = 0; i < 49; ++i) out->sh3[i] = (float)D3[i];
    return GSM_OK;
}

// bands of a scene's harmonics rows that the transform rotates: -1 when sh_components is none of 0, 1, 4, 9, 16
inline int transform_degree(uint32_t shComponents) {
    switch (shComponents) {
        case 0: case 1: return 0;
        case 4: return 1;
        case 9: return 2;
        case 16: return 3;
        default: return -1;
    }
}

// The fp16 row of 16 components is 96 bytes and is read and written as six 16-byte accesses, as the projection reads
// it: its base must be 16-byte aligned.  Every other row needs its element's alignment alone.
inline uint32_t transform_harmonics_alignment(bool half, uint32_t shComponents) {
    return half ? (shComponents == 16 ? 16u : 2u) : 4u;
}

// whether the rows go as 16-byte accesses: the row a multiple of 16 bytes and the base 16-byte aligned
inline bool transform_wide_rows(bool half, uint32_t shComponents, const void* harmonics) {
    return extract_harmonics_row_bytes(half, shComponents) % 16u == 0 && (((uintptr_t)harmonics) & 15u) == 0;
}

// gsm_global_transform's rows after the handle's, in the header's order
inline gsm_status transform_check(uint32_t maxGaussians, bool half, const gsm_global_scene* scene,
                                  const gsm_global_state* state, const uint32_t* keep,
                                  const gsm_global_transform_desc* desc) {
    // (the count of a NULL scene cannot be read: that is the missing buffer)
    if (scene && scene->gaussian_count > maxGaussians) return GSM_ERR_INVALID_GAUSSIAN_COUNT;
    if (!scene || !state || !keep || !desc) return GSM_ERR_MISSING_REQUIRED_BUFFER;
    const uint32_t count = scene->gaussian_count, sh = scene->sh_components;
    if (count > 0 && (!scene->gaussians || (sh > 1 && !scene->harmonics))) return GSM_ERR_MISSING_REQUIRED_BUFFER;
    if (((uintptr_t)scene->gaussians) & 15u) return GSM_ERR_INVALID_BUFFER_SIZE;
    if (sh > 1 && (((uintptr_t)scene->harmonics) & (transform_harmonics_alignment(half, sh) - 1u)))
        return GSM_ERR_INVALID_BUFFER_SIZE;
    if (state->default_state > 255u) return GSM_ERR_INVALID_ARGUMENT;
    if (transform_degree(sh) < 0) return GSM_ERR_INVALID_ARGUMENT;
    const float* f = reinterpret_cast<const float*>(desc);  // (the descriptor is 100 floats and nothing else)
    static_assert(sizeof(gsm_global_transform_desc) == 100 * sizeof(float), "the descriptor is 100 floats");
    for (int i = 0; i < 100; ++i)
        if (!std::isfinite(f[i])) return GSM_ERR_INVALID_ARGUMENT;
    if (!(desc->scale > 0.0f)) return GSM_ERR_INVALID_ARGUMENT;
    if (sh > 1 && ranges_meet(byte_range(scene->gaussians, count, extract_record_bytes(half)),
                              byte_range(scene->harmonics, count, extract_harmonics_row_bytes(half, sh))))
        return GSM_ERR_INVALID_ARGUMENT;
    return GSM_OK;
}

}  // namespace gsm
