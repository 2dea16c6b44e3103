// backward_gaussian.inc -- the body of k_preprocess_bwd and k_preprocess_bwd_planes (backward.hip),
// included once into each with `a` (GsrPreprocessBwdArgs, the kernel's argument), the constant kPlanes
// and dL_ddepths in scope.  Text, not a function template: the kernel without the flag is then
// compiled from the very statements it had before the planes (profiles/backward_resources.txt
// holds its registers line for line), where an inlined callee taking the arguments moved them.
// kPlanes: word 9 of the row is dL/dz through the planes' features; it goes to dL_ddepths
// (optional) and, z being the view matrix's z row applied to the mean, to dL_dmeans3D.
// kCamera (k_preprocess_bwd_camera, k_preprocess_bwd_planes_camera): the factors of the camera's
// gradient (gsr_backward_camera) go to `cam` (CameraTerms, zero on entry) on the way; the text is
// then the body of a lambda, so each `return` below leaves the lambda with cam's zeros or what
// was set so far and every thread of the block reaches the reduction after it.  Without the flag
// cam is not touched and the kernels compile as before.
// kAA (the four k_preprocess_bwd*_aa kernels, gsr_backward_filtered): the forward's opacity was
// o_eff = opacity s, s = sqrtf(fmaxf(0.000025f, rho)), rho = D0 / det with D0 the determinant
// before the 0.3 dilation; gop is dL/do_eff.  dL_dopacity = gop s and, off the floor, dL/drho =
// gop opacity / (2 s) joins the 2D covariance's gradient where the conic's becomes it.  Needs
// `opacities` in scope.  Without the flag the four kernels compile as before
// (profiles/antialias_resources.txt).
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.P) return;
    float *const sh_out = a.dL_dsh ? a.dL_dsh + idx * (int64_t)a.M * 3 : nullptr;
    if (a.radii[idx] <= 0) {  // culled by the forward: exact zeros
        store3(a.dL_dmeans3D, idx, 0.f, 0.f, 0.f);
        store3(a.dL_dmeans2D, idx, 0.f, 0.f, 0.f);
        if (a.dL_dopacity) a.dL_dopacity[idx] = 0.f;
        store3(a.dL_dcolors, idx, 0.f, 0.f, 0.f);
        store3(a.dL_dconic, idx, 0.f, 0.f, 0.f);
        store3(a.dL_dscales, idx, 0.f, 0.f, 0.f);
        if (a.dL_drotations)
            for (int i = 0; i < 4; ++i) a.dL_drotations[4 * idx + i] = 0.f;
        if (a.dL_dcov3D)
            for (int i = 0; i < 6; ++i) a.dL_dcov3D[6 * idx + i] = 0.f;
        if constexpr (kPlanes)
            if (dL_ddepths) dL_ddepths[idx] = 0.f;
        if (sh_out && a.sh_vec4) {
            for (int i = 0; i < 12; ++i)
                reinterpret_cast<float4 *>(sh_out)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        } else if (sh_out) {
            for (int i = 0; i < 3 * a.M; ++i) sh_out[i] = 0.f;
        }
        return;
    }
    const float *gr = a.grad2d + idx * kGradRow;
    const float gmx = gr[0], gmy = gr[1], gca = gr[2], gcb = gr[3], gcc = gr[4], gop = gr[5];
    const float grgb[3] = {gr[6], gr[7], gr[8]};
    // upstream's units: the gradient with respect to an offset added to the NDC centre
    const float gnx = gmx * (0.5f * (float)a.W), gny = gmy * (0.5f * (float)a.H);
    store3(a.dL_dmeans2D, idx, gnx, gny, 0.f);
    if constexpr (!kAA)
        if (a.dL_dopacity) a.dL_dopacity[idx] = gop;
    store3(a.dL_dcolors, idx, grgb[0], grgb[1], grgb[2]);
    store3(a.dL_dconic, idx, gca, gcb, gcc);

    const float *vm = a.viewmatrix, *pm = a.projmatrix;
    const float3 p = make_float3(a.means3D[3 * idx], a.means3D[3 * idx + 1], a.means3D[3 * idx + 2]);
    float dpx = 0.f, dpy = 0.f, dpz = 0.f;  // dL/dmeans3D

    // ---- the projective divide: ndc = hom.xy / (hom.w + 1e-7) --------------------------------
    {
        const float4 h = transform_point_4x4(p, pm);
        const float pw = 1.0f / (h.w + 0.0000001f);
        const float dhx = gnx * pw, dhy = gny * pw;
        const float dhw = -(gnx * h.x + gny * h.y) * pw * pw;
        dpx += pm[0] * dhx + pm[1] * dhy + pm[3] * dhw;
        dpy += pm[4] * dhx + pm[5] * dhy + pm[7] * dhw;
        dpz += pm[8] * dhx + pm[9] * dhy + pm[11] * dhw;
        if constexpr (kCamera) cam.dh[0] = dhx, cam.dh[1] = dhy, cam.dh[2] = dhw;
    }

    // ---- the colour: rgb = max(sum_b basis_b(dir) sh_b + 0.5, 0), dir = (p - campos) / len -----
    if (a.shs) {
        const float *sh = a.shs + idx * (int64_t)a.M * 3;
        const int ncoef = (a.D + 1) * (a.D + 1);
        float dx = p.x - a.campos[0], dy = p.y - a.campos[1], dz = p.z - a.campos[2];
        const float len = sqrtf(dx * dx + dy * dy + dz * dz);
        dx = dx / len, dy = dy / len, dz = dz / len;
        float b[16], bx[16], by[16], bz[16];
        sh_basis(dx, dy, dz, b, bx, by, bz);
        // the coefficients of the active degree (the others read as 0), kept in registers; rows
        // of 16 coefficients at 16-B aligned pointers move as 12 float4 (a.sh_vec4), in and out
        float c[48];
        const int nflt = 3 * ncoef;
        if (a.sh_vec4) {
            const float4 *v = reinterpret_cast<const float4 *>(sh);
            float4 rowv[12];
#pragma unroll
            for (int i = 0; i < 12; ++i) rowv[i] = v[i];
#pragma unroll
            for (int i = 0; i < 12; ++i) {
                c[4 * i] = 4 * i < nflt ? rowv[i].x : 0.f;
                c[4 * i + 1] = 4 * i + 1 < nflt ? rowv[i].y : 0.f;
                c[4 * i + 2] = 4 * i + 2 < nflt ? rowv[i].z : 0.f;
                c[4 * i + 3] = 4 * i + 3 < nflt ? rowv[i].w : 0.f;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 48; ++i) c[i] = i < nflt ? sh[i] : 0.f;
        }
        float val[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (k < ncoef)
                for (int ch = 0; ch < 3; ++ch) val[ch] += b[k] * c[3 * k + ch];
        float G[3];  // max(v + 0.5, 0) passes nothing on its flat side
        for (int ch = 0; ch < 3; ++ch) G[ch] = (val[ch] + 0.5f < 0.0f) ? 0.0f : grgb[ch];
        float ddx = 0.f, ddy = 0.f, ddz = 0.f;  // dL/ddir
        float o[48];                            // dL/dsh: 0 above the active degree
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const bool on = k < ncoef;
            if (on) {
                const float m = G[0] * c[3 * k] + G[1] * c[3 * k + 1] + G[2] * c[3 * k + 2];
                ddx += bx[k] * m, ddy += by[k] * m, ddz += bz[k] * m;
            }
            for (int ch = 0; ch < 3; ++ch) o[3 * k + ch] = on ? b[k] * G[ch] : 0.f;
        }
        if (sh_out) {
            if (a.sh_vec4) {
                float4 *w = reinterpret_cast<float4 *>(sh_out);
#pragma unroll
                for (int i = 0; i < 12; ++i)
                    w[i] = make_float4(o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]);
            } else {
#pragma unroll
                for (int i = 0; i < 48; ++i)
                    if (i < 3 * a.M) sh_out[i] = o[i];
                for (int i = 48; i < 3 * a.M; ++i) sh_out[i] = 0.f;
            }
        }
        // dir = d / |d|: (I - dir dir^T) / len
        const float dot = dx * ddx + dy * ddy + dz * ddz;
        dpx += (ddx - dx * dot) / len;
        dpy += (ddy - dy * dot) / len;
        dpz += (ddz - dz * dot) / len;
        if constexpr (kCamera) {  // dir depends on p - campos: minus the mean's term
            cam.dc[0] = -((ddx - dx * dot) / len);
            cam.dc[1] = -((ddy - dy * dot) / len);
            cam.dc[2] = -((ddz - dz * dot) / len);
        }
    } else if (sh_out) {
        for (int i = 0; i < 3 * a.M; ++i) sh_out[i] = 0.f;
    }

    // ---- the 3D covariance --------------------------------------------------------------------
    float c6[6];
    float3 sc = make_float3(0.f, 0.f, 0.f);
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.cov3D_precomp) {
        for (int i = 0; i < 6; ++i) c6[i] = a.cov3D_precomp[6 * idx + i];
    } else {
        sc = make_float3(a.scales[3 * idx], a.scales[3 * idx + 1], a.scales[3 * idx + 2]);
        q = make_float4(a.rotations[4 * idx], a.rotations[4 * idx + 1], a.rotations[4 * idx + 2],
                        a.rotations[4 * idx + 3]);
        compute_cov3d(sc, a.scale_modifier, q, c6);
    }

    // ---- the conic: (c, -b, a) / det of cov2 = A V A^T + 0.3 I, A = J R (2 x 3) ----------------
    const float3 t = transform_point_4x3(p, vm);
    const float limx = 1.3f * a.tanfovx, limy = 1.3f * a.tanfovy;
    const float txtz = t.x / t.z, tytz = t.y / t.z;
    const float cx = fminf(limx, fmaxf(-limx, txtz)), cy = fminf(limy, fmaxf(-limy, tytz));
    const bool clx = cx != txtz, cly = cy != tytz;  // on the clamp's flat side
    const float tx = cx * t.z, ty = cy * t.z, tz = t.z;
    const float fx = a.focal_x, fy = a.focal_y;
    const float tz2 = tz * tz;
    const float J00 = fx / tz, J02 = -(fx * tx) / tz2, J11 = fy / tz, J12 = -(fy * ty) / tz2;
    // R[r][c] = vm[4 c + r] (the view rotation); A = J R
    float A0[3], A1[3];
    for (int c = 0; c < 3; ++c) {
        A0[c] = J00 * vm[4 * c] + J02 * vm[4 * c + 2];
        A1[c] = J11 * vm[4 * c + 1] + J12 * vm[4 * c + 2];
    }
    const float V[3][3] = {{c6[0], c6[1], c6[2]}, {c6[1], c6[3], c6[4]}, {c6[2], c6[4], c6[5]}};
    float VA0[3], VA1[3];  // V A^T
    for (int i = 0; i < 3; ++i) {
        VA0[i] = V[i][0] * A0[0] + V[i][1] * A0[1] + V[i][2] * A0[2];
        VA1[i] = V[i][0] * A1[0] + V[i][1] * A1[1] + V[i][2] * A1[2];
    }
    const float ca0 = A0[0] * VA0[0] + A0[1] * VA0[1] + A0[2] * VA0[2];  // before the dilation
    const float ca = ca0 + 0.3f;
    const float cb = A0[0] * VA1[0] + A0[1] * VA1[1] + A0[2] * VA1[2];
    const float cc0 = A1[0] * VA1[0] + A1[1] * VA1[1] + A1[2] * VA1[2];
    const float cc = cc0 + 0.3f;
    const float det = ca * cc - cb * cb;
    const float id2 = 1.0f / (det * det);
    // conic = (cc, -cb, ca) / det, det - ca cc = -cb^2
    float dca = (-cc * cc * gca + cb * cc * gcb - cb * cb * gcc) * id2;
    float dcc = (-cb * cb * gca + ca * cb * gcb - ca * ca * gcc) * id2;
    float dcb = (2.0f * cb * cc * gca - (ca * cc + cb * cb) * gcb + 2.0f * ca * cb * gcc) * id2;
    if constexpr (kAA) {
        const float det0 = ca0 * cc0 - cb * cb;
        const float rho = det0 / det;
        float s = sqrtf(0.000025f);
        if (rho > 0.000025f) {  // off the floor (a gate): s = sqrt(rho)
            s = sqrtf(rho);
            const float grho = gop * opacities[idx] / (2.0f * s);
            // rho = D0 / D: d/da' = (c' D - D0 c) / D^2, d/dc' = (a' D - D0 a) / D^2,
            // d/db = -2 b (D - D0) / D^2 (b the one stored entry, as dcb)
            dca += grho * (cc0 * det - det0 * cc) * id2;
            dcc += grho * (ca0 * det - det0 * ca) * id2;
            dcb += grho * (-2.0f * cb * (det - det0)) * id2;
        }
        if (a.dL_dopacity) a.dL_dopacity[idx] = gop * s;
    }
    const float hb = 0.5f * dcb;  // each off-diagonal of the symmetric dL/dcov2
    // dL/dV = A^T G2 A (an off-diagonal of V stands for two entries: twice in dL/dcov3D)
    float GA0[3], GA1[3];  // G2 A
    for (int c = 0; c < 3; ++c) {
        GA0[c] = dca * A0[c] + hb * A1[c];
        GA1[c] = hb * A0[c] + dcc * A1[c];
    }
    float dV[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) dV[i][j] = A0[i] * GA0[j] + A1[i] * GA1[j];
    const float d6[6] = {dV[0][0], 2.0f * dV[0][1], 2.0f * dV[0][2], dV[1][1], 2.0f * dV[1][2],
                         dV[2][2]};
    if (a.dL_dcov3D)
        for (int i = 0; i < 6; ++i) a.dL_dcov3D[6 * idx + i] = d6[i];
    // dL/dA = 2 G2 A V, dL/dJ = dL/dA R^T
    float dA0[3], dA1[3];
    for (int c = 0; c < 3; ++c) {
        dA0[c] = 2.0f * (dca * VA0[c] + hb * VA1[c]);
        dA1[c] = 2.0f * (hb * VA0[c] + dcc * VA1[c]);
    }
    const float dJ00 = dA0[0] * vm[0] + dA0[1] * vm[4] + dA0[2] * vm[8];
    const float dJ02 = dA0[0] * vm[2] + dA0[1] * vm[6] + dA0[2] * vm[10];
    const float dJ11 = dA1[0] * vm[1] + dA1[1] * vm[5] + dA1[2] * vm[9];
    const float dJ12 = dA1[0] * vm[2] + dA1[1] * vm[6] + dA1[2] * vm[10];
    const float tz3 = tz2 * tz;
    float dtz = -fx / tz2 * dJ00 - fy / tz2 * dJ11 + 2.0f * fx * tx / tz3 * dJ02 +
                2.0f * fy * ty / tz3 * dJ12;
    const float dtxc = -fx / tz2 * dJ02, dtyc = -fy / tz2 * dJ12;  // d/d(clamped t.x, t.y)
    // t.x' = clamp(t.x / t.z) t.z, as written: (t.x / t.z) t.z inside (d/dt.x = 1, d/dt.z = 0),
    // +-lim t.z on the flat side (d/dt.x = 0, d/dt.z = +-lim)
    const float dtx = clx ? 0.0f : dtxc, dty = cly ? 0.0f : dtyc;
    dtz += (clx ? cx * dtxc : 0.0f) + (cly ? cy * dtyc : 0.0f);
    dpx += vm[0] * dtx + vm[1] * dty + vm[2] * dtz;
    dpy += vm[4] * dtx + vm[5] * dty + vm[6] * dtz;
    dpz += vm[8] * dtx + vm[9] * dty + vm[10] * dtz;
    if constexpr (kPlanes) {  // z = vm[2] x + vm[6] y + vm[10] z_world + vm[14]
        const float gz = gr[9];
        if (dL_ddepths) dL_ddepths[idx] = gz;
        dpx += vm[2] * gz, dpy += vm[6] * gz, dpz += vm[10] * gz;
    }
    store3(a.dL_dmeans3D, idx, dpx, dpy, dpz);
    if constexpr (kCamera) {
        cam.q[0] = p.x, cam.q[1] = p.y, cam.q[2] = p.z, cam.q[3] = 1.0f;
        cam.dt[0] = dtx, cam.dt[1] = dty, cam.dt[2] = dtz;
        if constexpr (kPlanes) cam.dt[2] += gr[9];  // z = t.z
        for (int c = 0; c < 3; ++c) cam.dA0[c] = dA0[c], cam.dA1[c] = dA1[c];
        cam.J[0] = J00, cam.J[1] = J02, cam.J[2] = J11, cam.J[3] = J12;
    }

    // ---- Sigma = N N^T, N = Rq diag(mod s) (the rotation as given, not renormalised) ------------
    if (a.cov3D_precomp) {
        store3(a.dL_dscales, idx, 0.f, 0.f, 0.f);
        if (a.dL_drotations)
            for (int i = 0; i < 4; ++i) a.dL_drotations[4 * idx + i] = 0.f;
        return;
    }
    const float r = q.x, x = q.y, y = q.z, z = q.w;
    const float Rq[3][3] = {
        {1.f - 2.f * (y * y + z * z), 2.f * (x * y - r * z), 2.f * (x * z + r * y)},
        {2.f * (x * y + r * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z - r * x)},
        {2.f * (x * z - r * y), 2.f * (y * z + r * x), 1.f - 2.f * (x * x + y * y)}};
    const float sm[3] = {a.scale_modifier * sc.x, a.scale_modifier * sc.y, a.scale_modifier * sc.z};
    float ds[3], D[3][3];  // dL/ds, dL/dRq
    for (int j = 0; j < 3; ++j) {
        ds[j] = 0.f;
        for (int i = 0; i < 3; ++i) {
            // dL/dN[i][j] = 2 (dV N)[i][j], N[k][j] = Rq[k][j] sm[j]
            const float dN = 2.0f * sm[j] *
                             (dV[i][0] * Rq[0][j] + dV[i][1] * Rq[1][j] + dV[i][2] * Rq[2][j]);
            ds[j] += dN * Rq[i][j];
            D[i][j] = dN * sm[j];
        }
        ds[j] *= a.scale_modifier;
    }
    store3(a.dL_dscales, idx, ds[0], ds[1], ds[2]);
    if (a.dL_drotations) {
        float *o = a.dL_drotations + 4 * idx;
        o[0] = 2.f * (-z * D[0][1] + y * D[0][2] + z * D[1][0] - x * D[1][2] - y * D[2][0] +
                      x * D[2][1]);
        o[1] = 2.f * (y * D[0][1] + z * D[0][2] + y * D[1][0] - 2.f * x * D[1][1] - r * D[1][2] +
                      z * D[2][0] + r * D[2][1] - 2.f * x * D[2][2]);
        o[2] = 2.f * (-2.f * y * D[0][0] + x * D[0][1] + r * D[0][2] + x * D[1][0] + z * D[1][2] -
                      r * D[2][0] + z * D[2][1] - 2.f * y * D[2][2]);
        o[3] = 2.f * (-2.f * z * D[0][0] - r * D[0][1] + x * D[0][2] + r * D[1][0] -
                      2.f * z * D[1][1] + y * D[1][2] + x * D[2][0] + y * D[2][1]);
    }
