// gs_bwd_chain.h -- the per-splat part of a frame's backward, written once (device): from the summed row of a splat back
// through the frame's per-splat expressions (conic <- 2-D covariance <- scale, rotation and the view; screen position and
// depth <- view-space position; colour <- SH basis <- direction).  One function, bwd_chain<CAMERA>, serves the record
// gradient of gs_backward.hip (CAMERA = false) and the camera gradient of gs_camera.hip (CAMERA = true).
#pragma once

#include "gs_splat_math.h"

namespace gs {

// Common.glsl:94-138 as a function of (X, Y, Z) = (-dx, -dy, dz), with its partial derivatives
__device__ __forceinline__ void sh_basis_grad(float X, float Y, float Z, float b[16], float bx[16], float by[16], float bz[16]) {
    const float S1 = 2.0f * X * Y, C1 = X * X - Y * Y;
    const float S2 = X * S1 + Y * C1, C2 = X * C1 - Y * S1;
    const float Z2 = Z * Z;
#pragma unroll
    for (int k = 0; k < 16; ++k) { bx[k] = 0.0f; by[k] = 0.0f; bz[k] = 0.0f; }
    b[0] = 0.2820947917738781f;
    b[1] = -0.48860251190292f * Y;                  by[1] = -0.48860251190292f;
    b[2] = 0.4886025119029199f * Z;                 bz[2] = 0.4886025119029199f;
    b[3] = -0.48860251190292f * X;                  bx[3] = -0.48860251190292f;
    b[4] = 0.5462742152960395f * S1;                bx[4] = 0.5462742152960395f * 2.0f * Y; by[4] = 0.5462742152960395f * 2.0f * X;
    b[5] = -1.092548430592079f * Z * Y;             by[5] = -1.092548430592079f * Z; bz[5] = -1.092548430592079f * Y;
    b[6] = 0.9461746957575601f * Z2 + -0.31539156525252f;   bz[6] = 0.9461746957575601f * 2.0f * Z;
    b[7] = -1.092548430592079f * Z * X;             bx[7] = -1.092548430592079f * Z; bz[7] = -1.092548430592079f * X;
    b[8] = 0.5462742152960395f * C1;                bx[8] = 0.5462742152960395f * 2.0f * X; by[8] = 0.5462742152960395f * -2.0f * Y;
    b[9] = -0.5900435899266435f * S2;               bx[9] = -0.5900435899266435f * 6.0f * X * Y;
                                                    by[9] = -0.5900435899266435f * 3.0f * (X * X - Y * Y);
    b[10] = 1.445305721320277f * Z * S1;            bx[10] = 1.445305721320277f * Z * 2.0f * Y; by[10] = 1.445305721320277f * Z * 2.0f * X;
                                                    bz[10] = 1.445305721320277f * S1;
    const float tc = -2.285228997322329f * Z2 + 0.4570457994644658f, dtc = -2.285228997322329f * 2.0f * Z;
    b[11] = tc * Y;                                 by[11] = tc; bz[11] = dtc * Y;
    b[12] = Z * (1.865881662950577f * Z2 + -1.119528997770346f);
                                                    bz[12] = 3.0f * 1.865881662950577f * Z2 + -1.119528997770346f;
    b[13] = tc * X;                                 bx[13] = tc; bz[13] = dtc * X;
    b[14] = 1.445305721320277f * Z * C1;            bx[14] = 1.445305721320277f * Z * 2.0f * X; by[14] = 1.445305721320277f * Z * -2.0f * Y;
                                                    bz[14] = 1.445305721320277f * C1;
    b[15] = -0.5900435899266435f * C2;              bx[15] = -0.5900435899266435f * 3.0f * (X * X - Y * Y);
                                                    by[15] = -0.5900435899266435f * -6.0f * X * Y;
}

// From the summed row of a splat down the per-splat part of the frame, to dL/d(record) (CAMERA = false: gs_backward*) or
// to the splat's 35 camera terms (CAMERA = true: gs_backward_camera*).  The branch the forward took is held fixed: the clamp
// of x/z, y/z in getCovarianceMatrix (a clamped component passes no derivative to the ratio), max(colour, 0) (no derivative
// below 0), det == 0 (opacity 0: the splat never contributes, all zero), and in an anti-aliased frame the floor under
// det0 / det and the cap at 1 above it (there the factor is a constant: the opacity gets dop * rho, the covariance nothing).
// `row` = the summed row of splat g, `any` = g emitted into the list.  CAMERA = false: o = the quads of its record gradient
// (cg unused).  CAMERA = true: cg[0..15] receives dL/dview, cg[16..31] dL/dproj, cg[32..34] dL/dcam_pos of this splat
// (cg[35] arrives zeroed and stays so for a zero row; o unused); the view's bottom row (3, 7, 11, 15) and the
// projection's clip-z row (18, 22, 26, 30) are never written: the view is taken as affine, and no frame reads clip z.
// The record side is one body for the dense and the visible kernel -- the same expressions in the same order, so the same
// bits -- and the camera side adds nothing to it: every camera statement sits behind `if constexpr (CAMERA)`.
template <bool CAMERA>
__device__ __forceinline__ void bwd_chain(const FrameParams& fp, const SceneBuffers& scene, uint32_t g, bool any,
                                          const float (&row)[kRowFloats], float4* o, float* cg) {
    const uint32_t n = fp.num_gaussians;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (any) {
        bool nz = false;
#pragma unroll
        for (int k = 0; k < kRowFloats; ++k) nz = nz || row[k] != 0.0f;
        any = nz;
    }
    if (!any) {
        if constexpr (!CAMERA) {
#pragma unroll
            for (uint32_t k = 0; k < kRecordQuads; ++k) o[k] = zero4;
        }
        return;
    }
    const float dsx = row[0], dsy = row[1], dix = row[2], diy = row[3], diz = row[4];
    const float dcol[3] = {row[5], row[6], row[7]};
    const float dop = row[8], dz = row[9];
    const float p[3] = {scene.pos[g], scene.pos[(size_t)n + g], scene.pos[2 * (size_t)n + g]};
    float s[3], q[4];
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] = scene.scale[(size_t)k * n + g];
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = scene.rot[(size_t)k * n + g];
    const float qr = q[0], qx = q[1], qy = q[2], qz = q[3];

    float vp[4], cp[4];
    mat4_mul_vec4(fp.view, p[0], p[1], p[2], 1.0f, vp);
    mat4_mul_vec4(fp.proj, vp[0], vp[1], vp[2], vp[3], cp);
    float dvp[4] = {0.f, 0.f, 0.f, 0.f};

    // screen position (Common.glsl:80-89): s = ((+-ndc + 1) / 2) * extent, ndc = clip.xy / clip.w
    {
        const float dnx = dsx * 0.5f * (float)fp.width, dny = -dsy * 0.5f * (float)fp.height;
        const float rw = 1.0f / cp[3];
        const float dc[4] = {dnx * rw, dny * rw, 0.0f, -(dnx * cp[0] + dny * cp[1]) * rw * rw};
#pragma unroll
        for (int c = 0; c < 4; ++c)
            dvp[c] += fp.proj[c * 4 + 0] * dc[0] + fp.proj[c * 4 + 1] * dc[1] + fp.proj[c * 4 + 3] * dc[3];
        if constexpr (CAMERA) {                             // clip = proj * vp, rows 0, 1 and 3
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                cg[16 + c * 4 + 0] = dc[0] * vp[c];
                cg[16 + c * 4 + 1] = dc[1] * vp[c];
                cg[16 + c * 4 + 3] = dc[3] * vp[c];
            }
        }
    }
    dvp[2] += -dz;                                          // depth = -viewSpacePos.z

    // 2-D covariance (Common.glsl:32-78) and its inverse (RenderGaussians.comp:94-107)
    const Mat3 rm = get_rot_mat(qr, qx, qy, qz);            // R[row][col] of getRotMat = rm.m[col][row]
    float M[3][3], Sg[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) M[i][k] = rm.m[k][i] * s[k];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Sg[i][j] = M[i][0] * M[j][0] + M[i][1] * M[j][1] + M[i][2] * M[j][2];
    const float wdt = (float)fp.width, hgt = (float)fp.height;
    const float tfy = fp.tan_fov_y, tfx = tfy * wdt / hgt;
    const float fx = wdt / (2.0f * tfx), fy = hgt / (2.0f * tfy);
    const float lim_x = tfx * fp.in_view_limit, lim_y = tfy * fp.in_view_limit;
    const float tz = vp[2];
    const float rx = vp[0] / tz, ry = vp[1] / tz;
    const bool clamp_x = rx < -lim_x || rx > lim_x, clamp_y = ry < -lim_y || ry > lim_y;
    const float ux = clampf(rx, -lim_x, lim_x), uy = clampf(ry, -lim_y, lim_y);
    const float pvx = ux * tz, pvy = uy * tz;
    const float J00 = fx / tz, J11 = fy / tz, J02 = -(fx * pvx) / (tz * tz), J12 = -(fy * pvy) / (tz * tz);
    float W[3][3], Tm[2][3];                                // W[row][col] = view; T = J W (its third row is zero)
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) W[r][c] = fp.view[c * 4 + r];
#pragma unroll
    for (int c = 0; c < 3; ++c) { Tm[0][c] = J00 * W[0][c] + J02 * W[2][c]; Tm[1][c] = J11 * W[1][c] + J12 * W[2][c]; }
    float TS[2][3];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) TS[r][c] = Tm[r][0] * Sg[0][c] + Tm[r][1] * Sg[1][c] + Tm[r][2] * Sg[2][c];
    const float a0 = TS[0][0] * Tm[0][0] + TS[0][1] * Tm[0][1] + TS[0][2] * Tm[0][2];      // before the 0.3 dilation
    const float cb = TS[1][0] * Tm[0][0] + TS[1][1] * Tm[0][1] + TS[1][2] * Tm[0][2];
    const float c0 = TS[1][0] * Tm[1][0] + TS[1][1] * Tm[1][1] + TS[1][2] * Tm[1][2];
    const float ca = a0 + 0.3f, cc = c0 + 0.3f;
    const float det = ca * cc - cb * cb;

    float dpos[3] = {0.f, 0.f, 0.f}, dscale[3] = {0.f, 0.f, 0.f}, drot[4] = {0.f, 0.f, 0.f, 0.f};
    float dop_rec = dop;                                    // dL/d(the record's opacity)
    if (det != 0.0f) {
        const float rd = 1.0f / det;
        const float ix = cc * rd, iy = -cb * rd, iz = ca * rd;
        const float ddet = -(dix * ix + diy * iy + diz * iz) * rd;
        float da = diz * rd + ddet * cc, db = -diy * rd - 2.0f * cb * ddet, dcc = dix * rd + ddet * ca;
        // an anti-aliased frame (gs_set_antialias) blended opacity * rho, rho = sqrt(max(r, floor)), r = det0 / det: the
        // record's opacity gets dop * rho, and above the floor dop * opacity flows on through r into the covariance
        if (fp.antialias) {
            const float det0 = a0 * c0 - cb * cb;
            const float r = det0 / det;
            const bool above = r > kAntialiasFloor;         // false for a NaN r, as in k_project
            const float rho = sqrtf(above ? (r < 1.0f ? r : 1.0f) : kAntialiasFloor);
            dop_rec = dop * rho;
            if (above && r <= 1.0f) {                       // beyond 1 (rounding alone) k_project capped the factor: a constant too
                const float drho = dop * scene.opacity[g];
                const float dr = drho / (2.0f * rho);
                const float ddet0 = dr / det, ddet_r = -dr * r / det;
                da += ddet0 * c0 + ddet_r * cc;
                dcc += ddet0 * a0 + ddet_r * ca;
                db += -2.0f * cb * (ddet0 + ddet_r);
            }
        }
        const float Gs[2][2] = {{2.0f * da, db}, {db, 2.0f * dcc}};   // dL/dSigma' + its transpose (upper 2 x 2)
        float GT[2][3];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) GT[r][c] = Gs[r][0] * Tm[0][c] + Gs[r][1] * Tm[1][c];
        // dL/dT = Gs T Sigma;  dL/dM = (T^T Gs T) M
        float dT[2][3], dSs[3][3];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) dT[r][c] = GT[r][0] * Sg[0][c] + GT[r][1] * Sg[1][c] + GT[r][2] * Sg[2][c];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) dSs[i][j] = Tm[0][i] * GT[0][j] + Tm[1][i] * GT[1][j];
        float dR[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float dM = dSs[i][0] * M[0][k] + dSs[i][1] * M[1][k] + dSs[i][2] * M[2][k];
                dR[i][k] = dM * s[k];
                dscale[k] += dM * rm.m[k][i];
            }
        // getRotMat's entries as functions of (r, x, y, z)
        drot[0] = 2.0f * (-qz * dR[1][0] + qy * dR[2][0] + qz * dR[0][1] - qx * dR[2][1] - qy * dR[0][2] + qx * dR[1][2]);
        drot[1] = 2.0f * (qy * dR[1][0] + qz * dR[2][0] + qy * dR[0][1] - 2.0f * qx * dR[1][1] - qr * dR[2][1] +
                          qz * dR[0][2] + qr * dR[1][2] - 2.0f * qx * dR[2][2]);
        drot[2] = 2.0f * (-2.0f * qy * dR[0][0] + qx * dR[1][0] + qr * dR[2][0] + qx * dR[0][1] + qz * dR[2][1] -
                          qr * dR[0][2] + qz * dR[1][2] - 2.0f * qy * dR[2][2]);
        drot[3] = 2.0f * (-2.0f * qz * dR[0][0] - qr * dR[1][0] + qx * dR[2][0] + qr * dR[0][1] - 2.0f * qz * dR[1][1] +
                          qy * dR[2][1] + qx * dR[0][2] + qy * dR[1][2]);
        if constexpr (CAMERA) {                             // T = J W, W the view's rotation block: dL/dW = J^T dL/dT
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                cg[c * 4 + 0] = J00 * dT[0][c];
                cg[c * 4 + 1] = J11 * dT[1][c];
                cg[c * 4 + 2] = J02 * dT[0][c] + J12 * dT[1][c];
            }
        }
        // dL/dJ = dL/dT W^T, then J's dependence on the view-space position
        float dJ[2][3];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int k = 0; k < 3; ++k) dJ[r][k] = dT[r][0] * W[k][0] + dT[r][1] * W[k][1] + dT[r][2] * W[k][2];
        const float tz2 = tz * tz, tz3 = tz2 * tz;
        float dtz = -fx / tz2 * dJ[0][0] - fy / tz2 * dJ[1][1] + 2.0f * fx * pvx / tz3 * dJ[0][2] + 2.0f * fy * pvy / tz3 * dJ[1][2];
        const float dpvx = -fx / tz2 * dJ[0][2], dpvy = -fy / tz2 * dJ[1][2];
        // pv.x = clamp(x / z) * z: d/dx = 1, d/dz = 0 inside the limits; d/dx = 0, d/dz = +-limit on the clamp
        if (clamp_x) dtz += dpvx * ux; else dvp[0] += dpvx;
        if (clamp_y) dtz += dpvy * uy; else dvp[1] += dpvy;
        dvp[2] += dtz;
    }

    // colour (Common.glsl:141-170, InitSortList.comp:124-126)
    const float ddx = p[0] - fp.cam_pos[0], ddy = p[1] - fp.cam_pos[1], ddz = p[2] - fp.cam_pos[2];
    const float len = sqrtf(ddx * ddx + ddy * ddy + ddz * ddz);
    const float dir[3] = {ddx / len, ddy / len, ddz / len};
    float b[16], bx[16], by[16], bz[16];
    sh_basis_grad(-dir[0], -dir[1], dir[2], b, bx, by, bz);
    // the coefficients [k_lo, k_hi) the frame's sh_mode uses (5 = GS_SH_DEGREE_1: 4, 4 = GS_SH_DEGREE_2: 9); no other plane is read
    const int k_lo = fp.sh_mode == 1u ? 1 : 0;
    const int k_hi = fp.sh_mode == 2u ? 1 : fp.sh_mode == 5u ? 4 : fp.sh_mode == 4u ? 9 : 16;
    float dres[3];
    {
        const float* shp = scene.sh + g;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float res = 0.0f;
            for (int k = k_lo; k < k_hi; ++k) res += shp[(size_t)(k * 3 + c) * n] * b[k];
            if (fp.sh_mode == 1u) res -= 0.5f;
            res += 0.5f;
            dres[c] = res >= 0.0f ? dcol[c] : 0.0f;                     // max(colour, 0)
        }
        float dX = 0.f, dY = 0.f, dZ = 0.f;
        if (fp.sh_mode != 2u) {
            for (int k = k_lo; k < k_hi; ++k) {
                const float db_k = dres[0] * shp[(size_t)(k * 3 + 0) * n] + dres[1] * shp[(size_t)(k * 3 + 1) * n] +
                                   dres[2] * shp[(size_t)(k * 3 + 2) * n];
                dX += db_k * bx[k]; dY += db_k * by[k]; dZ += db_k * bz[k];
            }
        }
        const float dd[3] = {-dX, -dY, dZ};                              // d/d(dir)
        const float dot = dd[0] * dir[0] + dd[1] * dir[1] + dd[2] * dir[2];
#pragma unroll
        for (int k = 0; k < 3; ++k) dpos[k] += (dd[k] - dir[k] * dot) / len;
        if constexpr (CAMERA) {                             // the direction starts at cam_pos: minus the position's term
#pragma unroll
            for (int k = 0; k < 3; ++k) cg[32 + k] = fp.sh_mode != 2u ? -dpos[k] : 0.0f;
        }
    }
    if constexpr (CAMERA) {                                 // vp = view * (p, 1): the final dvp against (p, 1), on top of dW
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) cg[c * 4 + r] += dvp[r] * p[c];
            cg[12 + r] = dvp[r];
        }
        return;
    }
    // view-space position <- world position
#pragma unroll
    for (int k = 0; k < 3; ++k)
        dpos[k] += fp.view[k * 4 + 0] * dvp[0] + fp.view[k * 4 + 1] * dvp[1] + fp.view[k * 4 + 2] * dvp[2] + fp.view[k * 4 + 3] * dvp[3];

    o[kRecPos / 4] = make_float4(dpos[0], dpos[1], dpos[2], 0.0f);
    o[kRecScale / 4] = make_float4(dscale[0], dscale[1], dscale[2], 0.0f);
    o[kRecRot / 4] = make_float4(drot[0], drot[1], drot[2], drot[3]);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const bool used = k >= k_lo && k < k_hi;
        o[kRecSh / 4 + k] = make_float4(used ? dres[0] * b[k] : 0.0f, used ? dres[1] * b[k] : 0.0f,
                                        used ? dres[2] * b[k] : 0.0f, k == 0 ? dop_rec : 0.0f);     // .w of k = 0: the opacity
    }
    o[kRecColor / 4] = zero4;
    o[kRecCov / 4] = zero4;
}

} // namespace gs
