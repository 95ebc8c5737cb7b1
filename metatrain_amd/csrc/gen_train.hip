// Size-generic PET TRAINING pass (SURVEY §8 row a16 for every model the tuned second-order pass of so.hip does not serve:
// other model sizes, d_node == d_pet, PostLN transformer layers, the residual featuriser -- VERDICT r2 missing #1 / #3).
//
// What the reference gets from `loss.backward()` after `autograd.grad(E, R, create_graph=True)` (pet/trainer.py:417-467,
// utils/output_gradient.py:34-40) is computed as FORWARD-OVER-REVERSE on "dual" activations, like so.hip but unfused and
// with run-time sizes:  with u = dL_F/d(dE/dR) the tangent of every edge vector is v'_p = u_j - u_i (+ S cell'), and
//     <u, dE/dR> = d/d eps sum_i lambda_i e_i(R + eps u) = sum_i lambda_i e'_i,
//     dL/d theta = d/d theta J,   J = sum_i (nu_i e_i + lambda_i e'_i),   nu_i = dL_E/d e_i, lambda_i = the force pass' seeds.
// Sweep 1 evaluates every stage on (x, x') pairs -- each Linear once on the primal and once (without bias) on the tangent
// rows, each non-linearity with its derivative; sweep 2 walks back with two adjoints per activation, (nu_x, lambda_x) =
// dJ/d(x, x'), and at every Linear adds  dW += nu_y^T x + lambda_y^T x',  db += sum nu_y.  The second-order identities of
// RMSNorm / LayerNorm, SiLU, SwiGLU and soft-max attention used here were checked against torch.autograd in fp64 before
// the kernels were written (1e-16). Weight-gradient reductions run over row chunks into partial buffers that a second
// kernel sums in a fixed order: no float atomics, bit-reproducible. Correctness-first: fp32 FMA, nothing fused.
#include <map>
#include <string>

#include "gen_walk.h"
#include "cutoff.h"
#include "long_range.h"

namespace pet {


namespace {

// ---------------------------------------------------------------------------------------------
// geometry tangents: geo' = (v', d'), fc', b' = (log max(fc, 1e-15))'
// ---------------------------------------------------------------------------------------------
__global__ void k_gt_geo(const float4* __restrict__ geo, const float* __restrict__ d0, const float* __restrict__ fc,
                         const int* __restrict__ ctr, const int* __restrict__ nbr, const int* __restrict__ shift,
                         const int* __restrict__ sys, const float* __restrict__ u, const float* __restrict__ ucell,
                         float4* __restrict__ geod, float* __restrict__ fcd, float* __restrict__ bd, int64_t E, float cutoff,
                         float width, int fn) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= E) return;
    const int i = ctr[p], j = nbr[p];
    float vx = u[3 * j] - u[3 * i], vy = u[3 * j + 1] - u[3 * i + 1], vz = u[3 * j + 2] - u[3 * i + 2];
    if (ucell) {   // v = r_j - r_i + S cell: the cell tangent of the stress term (utils/evaluate_model.py:305-321)
        const float* c = ucell + 9 * (int64_t)sys[i];
        const float sa = (float)shift[3 * p], sb = (float)shift[3 * p + 1], sc = (float)shift[3 * p + 2];
        vx += sa * c[0] + sb * c[3] + sc * c[6];
        vy += sa * c[1] + sb * c[4] + sc * c[7];
        vz += sa * c[2] + sb * c[5] + sc * c[8];
    }
    const float4 g = geo[p];
    const float dot = g.x * vx + g.y * vy + g.z * vz;
    geod[p] = make_float4(vx, vy, vz, dot / g.w);                      // d sqrt(v.v + 1e-15) = v.v' / dist
    const float nrm = sqrtf(g.x * g.x + g.y * g.y + g.z * g.z);
    const float f = nrm > 0.f ? cutoff_deriv_dev(d0[p], cutoff, width, fn) * dot / nrm : 0.f;
    fcd[p] = f;
    bd[p] = fc[p] > 1e-15f ? f / fc[p] : 0.f;
}

// ---------------------------------------------------------------------------------------------
// dual row kernels
// ---------------------------------------------------------------------------------------------
// (y, y') = norm(x, x'):  y = gamma xhat + beta,  y' = gamma rstd (c' - xhat mean(xhat c'))
__global__ void k_gt_norm(const float* __restrict__ Xp, const float* __restrict__ Xt, const float* __restrict__ gamma,
                          const float* __restrict__ beta, int ln, float eps, float* __restrict__ Yp, float* __restrict__ Yt,
                          int64_t R, int W) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= R) return;
    const float* x = Xp + r * W;
    const float* xt = Xt + r * W;
    float mean = 0.f, meant = 0.f;
    if (ln) {
        float s = 0.f, st = 0.f;
        for (int k = lane; k < W; k += 64) { s += x[k]; st += xt[k]; }
        mean = wave_sum(s) / W;
        meant = wave_sum(st) / W;
    }
    float s2 = 0.f, s3 = 0.f;
    for (int k = lane; k < W; k += 64) {
        const float c = x[k] - mean;
        s2 += c * c;
        s3 += c * (xt[k] - meant);
    }
    const float rstd = 1.0f / sqrtf(wave_sum(s2) / W + eps);
    const float m = rstd * wave_sum(s3) / W;   // mean(xhat c')
    for (int k = lane; k < W; k += 64) {
        const float xh = (x[k] - mean) * rstd;
        Yp[r * W + k] = xh * gamma[k] + (beta ? beta[k] : 0.f);
        Yt[r * W + k] = gamma[k] * rstd * ((xt[k] - meant) - xh * m);
    }
}

// (nu_x, lambda_x) (+)= adjoint of k_gt_norm for (nu_y, lambda_y); G (optional) receives nu_y xhat + lambda_y xhat' (its
// column sum is d gamma)
__global__ void k_gt_norm_rev(const float* __restrict__ Xp, const float* __restrict__ Xt, const float* __restrict__ gamma,
                              int ln, float eps, const float* __restrict__ NYp, const float* __restrict__ NYt,
                              float* __restrict__ NXp, float* __restrict__ NXt, int acc, float* __restrict__ G, int64_t R,
                              int W) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= R) return;
    const float* x = Xp + r * W;
    const float* xt = Xt + r * W;
    const float* ny = NYp + r * W;
    const float* ly = NYt + r * W;
    const float iw = 1.0f / W;
    float mean = 0.f, meant = 0.f;
    if (ln) {
        float s = 0.f, st = 0.f;
        for (int k = lane; k < W; k += 64) { s += x[k]; st += xt[k]; }
        mean = wave_sum(s) * iw;
        meant = wave_sum(st) * iw;
    }
    float s2 = 0.f, s3 = 0.f;
    for (int k = lane; k < W; k += 64) {
        const float c = x[k] - mean;
        s2 += c * c;
        s3 += c * (xt[k] - meant);
    }
    const float rstd = 1.0f / sqrtf(wave_sum(s2) * iw + eps);
    const float m = rstd * wave_sum(s3) * iw;
    // s_q = mean(q xhat), rbar = sum q xhat' / rstd, with p = gamma nu_y, q = gamma lambda_y
    float a_sq = 0.f, a_rb = 0.f;
    for (int k = lane; k < W; k += 64) {
        const float xh = (x[k] - mean) * rstd, cd = xt[k] - meant, q = gamma[k] * ly[k];
        a_sq += q * xh;
        a_rb += q * (cd - xh * m);   // = q xhat' / rstd
    }
    const float sq = wave_sum(a_sq) * iw, rb = wave_sum(a_rb);
    // xhat_bar = p - rstd (m q + s_q c');  t1 = mean(xhat_bar xhat)
    float a_t1 = 0.f;
    for (int k = lane; k < W; k += 64) {
        const float xh = (x[k] - mean) * rstd, cd = xt[k] - meant;
        const float xb = gamma[k] * ny[k] - rstd * (m * gamma[k] * ly[k] + sq * cd);
        a_t1 += xb * xh;
    }
    const float t1 = wave_sum(a_t1) * iw;
    const float coef = rstd * rb * iw + t1;
    // c_bar = rstd xhat_bar - rstd xhat coef;  c'_bar = rstd (q - xhat s_q);  LayerNorm: minus their means
    float a_cb = 0.f, a_cdb = 0.f;
    if (ln) {
        for (int k = lane; k < W; k += 64) {
            const float xh = (x[k] - mean) * rstd, cd = xt[k] - meant, q = gamma[k] * ly[k];
            const float xb = gamma[k] * ny[k] - rstd * (m * q + sq * cd);
            a_cb += rstd * xb - rstd * xh * coef;
            a_cdb += rstd * (q - xh * sq);
        }
        a_cb = wave_sum(a_cb) * iw;
        a_cdb = wave_sum(a_cdb) * iw;
    }
    for (int k = lane; k < W; k += 64) {
        const float xh = (x[k] - mean) * rstd, cd = xt[k] - meant, q = gamma[k] * ly[k];
        const float xb = gamma[k] * ny[k] - rstd * (m * q + sq * cd);
        const float cb = rstd * xb - rstd * xh * coef - a_cb;
        const float cdb = rstd * (q - xh * sq) - a_cdb;
        if (acc) { NXp[r * W + k] += cb; NXt[r * W + k] += cdb; }
        else { NXp[r * W + k] = cb; NXt[r * W + k] = cdb; }
        if (G) G[r * W + k] = ny[k] * xh + ly[k] * rstd * (cd - xh * m);
    }
}

// silu: s = a sig(a), s' = silu'(a) a'
__global__ void k_gt_silu(const float* __restrict__ Ap, const float* __restrict__ At, float* __restrict__ Sp,
                          float* __restrict__ St, int64_t n) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const float a = Ap[idx], s = gsig(a);
    Sp[idx] = a * s;
    St[idx] = s * (1.f + a * (1.f - s)) * At[idx];
}
// nu_a = nu_s silu' + lambda_s silu'' a';  lambda_a = lambda_s silu'   (in place on the adjoint allowed)
__global__ void k_gt_silu_rev(const float* __restrict__ Ap, const float* __restrict__ At, const float* __restrict__ NSp,
                              const float* __restrict__ NSt, float* __restrict__ NAp, float* __restrict__ NAt, int64_t n) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const float a = Ap[idx], s = gsig(a);
    const float d1 = s * (1.f + a * (1.f - s)), d2 = s * (1.f - s) * (2.f + a * (1.f - 2.f * s));
    const float ns = NSp[idx], ls = NSt[idx];
    NAp[idx] = ns * d1 + ls * d2 * At[idx];
    NAt[idx] = ls * d1;
}
// SwiGLU: S = v sig(g), S' = v' sig + v sig' g'
__global__ void k_gt_swiglu(const float* __restrict__ VGp, const float* __restrict__ VGt, float* __restrict__ Sp,
                            float* __restrict__ St, int64_t R, int F) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= R * F) return;
    const int64_t r = idx / F;
    const int k = (int)(idx % F);
    const float v = VGp[r * 2 * F + k], g = VGp[r * 2 * F + F + k], vd = VGt[r * 2 * F + k], gd = VGt[r * 2 * F + F + k];
    const float s = gsig(g), s1 = s * (1.f - s);
    Sp[idx] = v * s;
    St[idx] = vd * s + v * s1 * gd;
}
__global__ void k_gt_swiglu_rev(const float* __restrict__ VGp, const float* __restrict__ VGt, const float* __restrict__ NSp,
                                const float* __restrict__ NSt, float* __restrict__ NVGp, float* __restrict__ NVGt, int64_t R,
                                int F) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= R * F) return;
    const int64_t r = idx / F;
    const int k = (int)(idx % F);
    const float v = VGp[r * 2 * F + k], g = VGp[r * 2 * F + F + k], vd = VGt[r * 2 * F + k], gd = VGt[r * 2 * F + F + k];
    const float s = gsig(g), s1 = s * (1.f - s), s2 = s1 * (1.f - 2.f * s);
    const float nu = NSp[idx], la = NSt[idx];
    NVGp[r * 2 * F + k] = nu * s + la * s1 * gd;
    NVGp[r * 2 * F + F + k] = nu * v * s1 + la * (vd * s1 + v * s2 * gd);
    NVGt[r * 2 * F + k] = la * s;
    NVGt[r * 2 * F + F + k] = la * v * s1;
}

// ---------------------------------------------------------------------------------------------
// attention on dual tokens
// ---------------------------------------------------------------------------------------------
template <int HDM>
__global__ __launch_bounds__(64) void k_gt_attn(const float* __restrict__ Qp, const float* __restrict__ Qt,
                                                const int* __restrict__ rowptr, const float* __restrict__ fc,
                                                const float* __restrict__ bd, float* __restrict__ AOp,
                                                float* __restrict__ AOt, float* __restrict__ LSE, float* __restrict__ MS,
                                                int64_t E, int D, int NH, int HD, float scale) {
    const int i = blockIdx.x, h = blockIdx.y, lane = threadIdx.x;
    const int p0 = rowptr[i], T = rowptr[i + 1] - p0 + 1;
    const int64_t ld = 3 * (int64_t)D;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int tq = t0 + lane;
        if (tq >= T) continue;
        const int64_t rq = tq == 0 ? E + i : (int64_t)p0 + tq - 1;
        float q[HDM], qd[HDM], A0[HDM], A1[HDM], A2[HDM];
#pragma unroll
        for (int d = 0; d < HDM; d++) {
            q[d] = d < HD ? Qp[rq * ld + h * HD + d] * scale : 0.f;
            qd[d] = d < HD ? Qt[rq * ld + h * HD + d] * scale : 0.f;
            A0[d] = 0.f; A1[d] = 0.f; A2[d] = 0.f;
        }
        float mx = -INFINITY, l = 0.f, sda = 0.f;
        for (int tk = 0; tk < T; tk++) {
            const int64_t rk = tk == 0 ? E + i : (int64_t)p0 + tk - 1;
            const float* kp = Qp + rk * ld + D + h * HD;
            const float* kt = Qt + rk * ld + D + h * HD;
            const float* vp = Qp + rk * ld + 2 * D + h * HD;
            const float* vt = Qt + rk * ld + 2 * D + h * HD;
            float s = tk == 0 ? 0.f : logf(fmaxf(fc[p0 + tk - 1], 1e-15f));
            float sd = tk == 0 ? 0.f : bd[p0 + tk - 1];
#pragma unroll
            for (int d = 0; d < HDM; d++)
                if (d < HD) { s = fmaf(q[d], kp[d], s); sd = fmaf(qd[d], kp[d], fmaf(q[d], kt[d], sd)); }
            const float mn = fmaxf(mx, s), c = expf(mx - mn), p = expf(s - mn);
            l = l * c + p;
            sda = sda * c + p * sd;
#pragma unroll
            for (int d = 0; d < HDM; d++)
                if (d < HD) {
                    A0[d] = A0[d] * c + p * vp[d];
                    A1[d] = A1[d] * c + p * sd * vp[d];
                    A2[d] = A2[d] * c + p * vt[d];
                }
            mx = mn;
        }
        const float il = 1.0f / l, m = sda * il;
#pragma unroll
        for (int d = 0; d < HDM; d++)
            if (d < HD) {
                AOp[rq * D + h * HD + d] = A0[d] * il;
                AOt[rq * D + h * HD + d] = (A1[d] - m * A0[d] + A2[d]) * il;
            }
        LSE[rq * NH + h] = mx + logf(l);
        MS[rq * NH + h] = m;
    }
}

// pass Q (lanes = queries): c_i = sum_k p_ik (B_i . v_k), d_i = sum_k p_ik pbar_ik, then (nu_q, lambda_q)
template <int HDM>
__global__ __launch_bounds__(64) void k_gt_attn_rev_q(const float* __restrict__ Qp, const float* __restrict__ Qt,
                                                      const float* __restrict__ NOp, const float* __restrict__ NOt,
                                                      const float* __restrict__ LSE, const float* __restrict__ MS,
                                                      const int* __restrict__ rowptr, const float* __restrict__ fc,
                                                      const float* __restrict__ bd, float* __restrict__ NQp,
                                                      float* __restrict__ NQt, float* __restrict__ CC, float* __restrict__ DD,
                                                      int64_t E, int D, int NH, int HD, float scale) {
    const int i = blockIdx.x, h = blockIdx.y, lane = threadIdx.x;
    const int p0 = rowptr[i], T = rowptr[i + 1] - p0 + 1;
    const int64_t ld = 3 * (int64_t)D;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int tq = t0 + lane;
        if (tq >= T) continue;
        const int64_t rq = tq == 0 ? E + i : (int64_t)p0 + tq - 1;
        float q[HDM], qd[HDM], A[HDM], B[HDM], qb[HDM], qdb[HDM];
#pragma unroll
        for (int d = 0; d < HDM; d++) {
            q[d] = d < HD ? Qp[rq * ld + h * HD + d] * scale : 0.f;
            qd[d] = d < HD ? Qt[rq * ld + h * HD + d] * scale : 0.f;
            A[d] = d < HD ? NOp[rq * D + h * HD + d] : 0.f;
            B[d] = d < HD ? NOt[rq * D + h * HD + d] : 0.f;
            qb[d] = 0.f; qdb[d] = 0.f;
        }
        const float lse = LSE[rq * NH + h], m = MS[rq * NH + h];
        float cc = 0.f, dd = 0.f;
        for (int pass = 0; pass < 3; pass++) {
            for (int tk = 0; tk < T; tk++) {
                const int64_t rk = tk == 0 ? E + i : (int64_t)p0 + tk - 1;
                const float* kp = Qp + rk * ld + D + h * HD;
                const float* kt = Qt + rk * ld + D + h * HD;
                const float* vp = Qp + rk * ld + 2 * D + h * HD;
                const float* vt = Qt + rk * ld + 2 * D + h * HD;
                float s = tk == 0 ? 0.f : logf(fmaxf(fc[p0 + tk - 1], 1e-15f));
                float sd = tk == 0 ? 0.f : bd[p0 + tk - 1];
                float pdb = 0.f, av = 0.f, bvd = 0.f;
#pragma unroll
                for (int d = 0; d < HDM; d++)
                    if (d < HD) {
                        s = fmaf(q[d], kp[d], s);
                        sd = fmaf(qd[d], kp[d], fmaf(q[d], kt[d], sd));
                        pdb = fmaf(B[d], vp[d], pdb);
                        av = fmaf(A[d], vp[d], av);
                        bvd = fmaf(B[d], vt[d], bvd);
                    }
                const float p = expf(s - lse);
                if (pass == 0) { cc += p * pdb; continue; }
                const float pb = av + bvd + pdb * (sd - m) - sd * cc;
                if (pass == 1) { dd += p * pb; continue; }
                const float sb = p * (pb - dd), sdb = p * (pdb - cc);
#pragma unroll
                for (int d = 0; d < HDM; d++)
                    if (d < HD) {
                        qb[d] = fmaf(sb, kp[d], fmaf(sdb, kt[d], qb[d]));
                        qdb[d] = fmaf(sdb, kp[d], qdb[d]);
                    }
            }
        }
#pragma unroll
        for (int d = 0; d < HDM; d++)
            if (d < HD) { NQp[rq * ld + h * HD + d] = qb[d] * scale; NQt[rq * ld + h * HD + d] = qdb[d] * scale; }
        CC[rq * NH + h] = cc;
        DD[rq * NH + h] = dd;
    }
}

// pass K (lanes = keys): (nu, lambda) of k and v. TAP (the Hessian-vector product): also the adjoints of the key's mask bias
// b = log max(fc, 1e-15) and of its tangent b', SB / SDB [NH][E] = sum over the queries of p (pbar - d_q) and p (pdb - c_q)
// (no `scale`: the bias enters the logit unscaled). A lane owns one key and walks ALL queries of the row, so the sums are
// complete whichever 64-key chunk the key sits in. TAP = false is the training pass' kernel, unchanged.
template <int HDM, bool TAP = false>
__global__ __launch_bounds__(64) void k_gt_attn_rev_k(const float* __restrict__ Qp, const float* __restrict__ Qt,
                                                      const float* __restrict__ NOp, const float* __restrict__ NOt,
                                                      const float* __restrict__ LSE, const float* __restrict__ MS,
                                                      const float* __restrict__ CC, const float* __restrict__ DD,
                                                      const int* __restrict__ rowptr, const float* __restrict__ fc,
                                                      const float* __restrict__ bd, float* __restrict__ NQp,
                                                      float* __restrict__ NQt, int64_t E, int D, int NH, int HD,
                                                      float scale, float* __restrict__ SB, float* __restrict__ SDB) {
    const int i = blockIdx.x, h = blockIdx.y, lane = threadIdx.x;
    const int p0 = rowptr[i], T = rowptr[i + 1] - p0 + 1;
    const int64_t ld = 3 * (int64_t)D;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int tk = t0 + lane;
        if (tk >= T) continue;
        const int64_t rk = tk == 0 ? E + i : (int64_t)p0 + tk - 1;
        float k[HDM], kd[HDM], v[HDM], vd[HDM], kb[HDM], kdb[HDM], vb[HDM], vdb[HDM];
#pragma unroll
        for (int d = 0; d < HDM; d++) {
            k[d] = d < HD ? Qp[rk * ld + D + h * HD + d] : 0.f;
            kd[d] = d < HD ? Qt[rk * ld + D + h * HD + d] : 0.f;
            v[d] = d < HD ? Qp[rk * ld + 2 * D + h * HD + d] : 0.f;
            vd[d] = d < HD ? Qt[rk * ld + 2 * D + h * HD + d] : 0.f;
            kb[d] = 0.f; kdb[d] = 0.f; vb[d] = 0.f; vdb[d] = 0.f;
        }
        const float bias = tk == 0 ? 0.f : logf(fmaxf(fc[p0 + tk - 1], 1e-15f));
        const float biasd = tk == 0 ? 0.f : bd[p0 + tk - 1];
        float tb = 0.f, tdb = 0.f;
        for (int tq = 0; tq < T; tq++) {
            const int64_t rq = tq == 0 ? E + i : (int64_t)p0 + tq - 1;
            const float* qp = Qp + rq * ld + h * HD;
            const float* qt = Qt + rq * ld + h * HD;
            const float* ap = NOp + rq * D + h * HD;
            const float* bp = NOt + rq * D + h * HD;
            float s = 0.f, sd = 0.f, pdb = 0.f, av = 0.f, bvd = 0.f;
#pragma unroll
            for (int d = 0; d < HDM; d++)
                if (d < HD) {
                    s = fmaf(qp[d], k[d], s);
                    sd = fmaf(qt[d], k[d], fmaf(qp[d], kd[d], sd));
                    pdb = fmaf(bp[d], v[d], pdb);
                    av = fmaf(ap[d], v[d], av);
                    bvd = fmaf(bp[d], vd[d], bvd);
                }
            s = s * scale + bias;
            sd = sd * scale + biasd;
            const float m = MS[rq * NH + h], cc = CC[rq * NH + h], dq = DD[rq * NH + h];
            const float p = expf(s - LSE[rq * NH + h]);
            const float pb = av + bvd + pdb * (sd - m) - sd * cc;
            const float sb = p * (pb - dq) * scale, sdb = p * (pdb - cc) * scale, pd = p * (sd - m);
            if constexpr (TAP) { tb += p * (pb - dq); tdb += p * (pdb - cc); }
#pragma unroll
            for (int d = 0; d < HDM; d++)
                if (d < HD) {
                    kb[d] = fmaf(sb, qp[d], fmaf(sdb, qt[d], kb[d]));
                    kdb[d] = fmaf(sdb, qp[d], kdb[d]);
                    vb[d] = fmaf(p, ap[d], fmaf(pd, bp[d], vb[d]));
                    vdb[d] = fmaf(p, bp[d], vdb[d]);
                }
        }
#pragma unroll
        for (int d = 0; d < HDM; d++)
            if (d < HD) {
                NQp[rk * ld + D + h * HD + d] = kb[d];
                NQt[rk * ld + D + h * HD + d] = kdb[d];
                NQp[rk * ld + 2 * D + h * HD + d] = vb[d];
                NQt[rk * ld + 2 * D + h * HD + d] = vdb[d];
            }
        if constexpr (TAP) if (tk > 0) {   // (the centre token carries no bias); p0 + tk - 1 < rowptr[i + 1] <= E
            SB[(int64_t)h * E + p0 + tk - 1] = tb;
            SDB[(int64_t)h * E + p0 + tk - 1] = tdb;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Hessian-vector product: the three taps of sweep 2 that reach the geometry, and the geometry kernel
// ---------------------------------------------------------------------------------------------
// tap 2, reduction: (db, db') (+)= sum over the heads, in head order, of one attention layer's SB / SDB
__global__ void k_hvp_bias_sum(const float* __restrict__ SB, const float* __restrict__ SDB, int NH, int64_t E,
                               float* __restrict__ db, float* __restrict__ dbd, int acc) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= E) return;
    float a = 0.f, b = 0.f;
    for (int h = 0; h < NH; h++) { a += SB[(int64_t)h * E + p]; b += SDB[(int64_t)h * E + p]; }
    db[p] = acc ? db[p] + a : a;
    dbd[p] = acc ? dbd[p] + b : b;
}
// tap 3: e_i = .. + sum_e fc_e ep_e, e'_i = .. + sum_e (fc'_e ep_e + fc_e ep'_e)  =>  dJ/dfc = nu_i ep + lambda_i ep',
// dJ/dfc' = lambda_i ep (summed over the readout layers in layer order)
__global__ void k_hvp_fc_adj(const float* __restrict__ nA, const float* __restrict__ lA, const int* __restrict__ ctr,
                             const float* __restrict__ epp, const float* __restrict__ ept, float* __restrict__ dfc,
                             float* __restrict__ dfcd, int acc, int64_t E) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= E) return;
    const int64_t i = ctr[p];
    const float n = nA ? nA[i] : 0.f, l = lA ? lA[i] : 0.f;
    const float a = n * epp[p] + l * ept[p], b = l * epp[p];
    dfc[p] = acc ? dfc[p] + a : a;
    dfcd[p] = acc ? dfcd[p] + b : b;
}
// the geometry kernel: the (nu, lambda) pairs of geo = (v, d), of the key bias b and of the cutoff factor fc folded into
// ONE dJ/dv per edge -- the reverse of exactly what k_gt_geo computes, with v' held fixed (it does not depend on R):
//   d = sqrt(v.v + 1e-15), d' = w / d (w = v.v'):     dd/dv = v / d,            dd'/dv = v'/d - w v / d^3
//   fc = f(d0), fc' = f'(d0) w / |v| (d0 = |v|):      dfc/dv = f' v / |v|,      dfc'/dv = f'' w v / |v|^2 + f' (v'/|v| - w v / |v|^3)
//   b = log max(fc, 1e-15), b' = fc' / fc:            both flat where fc <= 1e-15; else dJ/dfc += db / fc - db' fc' / fc^2,
//                                                     dJ/dfc' += db' / fc
// The lambda half of geo's adjoint (that of v' and d') multiplies quantities that do not move with R, except d' above.
// fc and fc' in the fold of b' are the fp32 values the dual forward used (k_gt_geo: fc' from the fp32 cutoff_deriv), while
// f' and f'' here are evaluated in double: the adjoint of the formulas, not of the forward's roundings -- they differ by
// the fp32 rounding of f' (1e-7 relative), far inside the bar.
// Written as a [E, 4] "dgeo" with a zero distance slot: the scatter backward_geometry_generic then passes it through.
__global__ void k_hvp_geo(const float4* __restrict__ geo, const float4* __restrict__ geod, const float* __restrict__ d0,
                          const float* __restrict__ fc, const float* __restrict__ fcd, const float4* __restrict__ ngeo,
                          const float4* __restrict__ lgeo, const float* __restrict__ db, const float* __restrict__ dbd,
                          const float* __restrict__ dfc, const float* __restrict__ dfcd, float4* __restrict__ dv, int64_t E,
                          float cutoff, float width, int fn) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= E) return;
    const float4 g = geo[p], gt = geod[p], ng = ngeo[p], lg = lgeo[p];
    const double vx = g.x, vy = g.y, vz = g.z, tx = gt.x, ty = gt.y, tz = gt.z, dist = g.w;
    const double w = vx * tx + vy * ty + vz * tz, nrm = sqrt(vx * vx + vy * vy + vz * vz);
    double af = dfc[p], afd = dfcd[p];
    const double f = fc[p], fd = fcd[p];
    if (fc[p] > 1e-15f) {
        af += (double)db[p] / f - (double)dbd[p] * fd / (f * f);
        afd += (double)dbd[p] / f;
    }
    // dJ/dv = ng.xyz + cv v + ct v'
    double cv = (double)ng.w / dist - (double)lg.w * w / (dist * dist * dist), ct = (double)lg.w / dist;
    if (nrm > 0.0) {
        double f1, f2;
        cutoff_deriv2(d0[p], cutoff, width, fn, &f1, &f2);
        cv += af * f1 / nrm + afd * (f2 * w / (nrm * nrm) - f1 * w / (nrm * nrm * nrm));
        ct += afd * f1 / nrm;
    }
    dv[p] = make_float4((float)(ng.x + cv * vx + ct * tx), (float)(ng.y + cv * vy + ct * ty), (float)(ng.z + cv * vz + ct * tz), 0.f);
}

// ---------------------------------------------------------------------------------------------
// weight gradients: G[o][i] = sum_r (A0[r][o] B0[r][i] + A1[r][o] B1[r][i]), rows split into chunks, partials summed by
// k_gt_reduce in chunk order
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gt_wgrad(const float* __restrict__ A0, const float* __restrict__ B0,
                                                  const float* __restrict__ A1, const float* __restrict__ B1, int64_t lda,
                                                  int64_t ldb, int64_t R, int NO, int KI, int64_t per,
                                                  float* __restrict__ part) {
    __shared__ float As[16][65], Bs[16][65];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int o0 = blockIdx.x * 64, i0 = blockIdx.y * 64;
    const int64_t lo = (int64_t)blockIdx.z * per, hi = lo + per < R ? lo + per : R;
    float acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) acc[a][b] = 0.f;
    for (int seg = 0; seg < 2; seg++) {
        const float* A = seg ? A1 : A0;
        const float* B = seg ? B1 : B0;
        if (!A) continue;
        for (int64_t r0 = lo; r0 < hi; r0 += 16) {
            __syncthreads();
            for (int idx = threadIdx.x; idx < 16 * 64; idx += 256) {
                const int rr = idx >> 6, cc = idx & 63;
                const int64_t r = r0 + rr;
                As[rr][cc] = (r < hi && o0 + cc < NO) ? A[r * lda + o0 + cc] : 0.f;
                Bs[rr][cc] = (r < hi && i0 + cc < KI) ? B[r * ldb + i0 + cc] : 0.f;
            }
            __syncthreads();
#pragma unroll
            for (int rr = 0; rr < 16; rr++) {
                float a[4], b[4];
#pragma unroll
                for (int q = 0; q < 4; q++) { a[q] = As[rr][ty + 16 * q]; b[q] = Bs[rr][tx + 16 * q]; }
#pragma unroll
                for (int x = 0; x < 4; x++)
#pragma unroll
                    for (int y = 0; y < 4; y++) acc[x][y] = fmaf(a[x], b[y], acc[x][y]);
            }
        }
    }
    float* out = part + (size_t)blockIdx.z * NO * KI;
#pragma unroll
    for (int x = 0; x < 4; x++) {
        const int o = o0 + ty + 16 * x;
        if (o >= NO) continue;
#pragma unroll
        for (int y = 0; y < 4; y++) {
            const int i = i0 + tx + 16 * y;
            if (i < KI) out[(size_t)o * KI + i] = acc[x][y];
        }
    }
}
// column sums of A [R][W] (bias gradients, norm weight gradients from a per-row product buffer): partial per chunk
__global__ void k_gt_colsum(const float* __restrict__ A, int64_t lda, int64_t R, int W, int64_t per, float* __restrict__ part) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= W) return;
    const int64_t lo = (int64_t)blockIdx.y * per, hi = lo + per < R ? lo + per : R;
    double s = 0.0;   // bias gradients are sums of signed adjoints that largely cancel
    for (int64_t r = lo; r < hi; r++) s += (double)A[r * lda + k];
    part[(size_t)blockIdx.y * W + k] = (float)s;
}
__global__ void k_gt_reduce(const float* __restrict__ part, int n_chunks, int64_t n, float* __restrict__ dst) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    double s = 0.0;
    for (int c = 0; c < n_chunks; c++) s += (double)part[(size_t)c * n + idx];
    dst[idx] += (float)s;
}
// embedding gradients: part[chunk][index[r]][k] += X[r][k] (one thread per column: no races), reduced like the others
__global__ void k_gt_embed_grad(const int* __restrict__ index, const float* __restrict__ X, int64_t ldx, int64_t R, int W,
                                int ns, int64_t per, float* __restrict__ part) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= W) return;
    const int64_t lo = (int64_t)blockIdx.y * per, hi = lo + per < R ? lo + per : R;
    float* out = part + (size_t)blockIdx.y * ns * W;
    for (int s = 0; s < ns; s++) out[(size_t)s * W + k] = 0.f;
    for (int64_t r = lo; r < hi; r++) out[(size_t)index[r] * W + k] += X[r * ldx + k];
}

// heads: e_i = np_i + sum_e fc_e ep_e,  e'_i = np'_i + sum_e (fc'_e ep_e + fc_e ep'_e)  (accumulated over readout layers)
__global__ void k_gt_atom_sum(const float* __restrict__ npp, const float* __restrict__ npt, const float* __restrict__ epp,
                              const float* __restrict__ ept, const float* __restrict__ fc, const float* __restrict__ fcd,
                              const int* __restrict__ rowptr, float* __restrict__ tangent, int acc, int64_t N) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    float st = npt[i];
    for (int e = rowptr[i]; e < rowptr[i + 1]; e++) st += fcd[e] * epp[e] + fc[e] * ept[e];
    (void)npp;
    if (acc) tangent[i] += st;
    else tangent[i] = st;
}
// seeds: nu_np = nA, lambda_np = lA;  nu_ep = nA fc + lA fc',  lambda_ep = lA fc
__global__ void k_gt_seeds(const float* __restrict__ nA, const float* __restrict__ lA, const int* __restrict__ ctr,
                           const float* __restrict__ fc, const float* __restrict__ fcd, float* __restrict__ nnp,
                           float* __restrict__ lnp, float* __restrict__ nep, float* __restrict__ lep, int64_t N, int64_t E) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < N) { nnp[idx] = nA ? nA[idx] : 0.f; lnp[idx] = lA ? lA[idx] : 0.f; }
    if (idx < E) {
        const int64_t i = ctr[idx];
        const float n = nA ? nA[i] : 0.f, l = lA ? lA[i] : 0.f;
        nep[idx] = n * fc[idx] + l * fcd[idx];
        lep[idx] = l * fc[idx];
    }
}

// further targets (first order, P properties): the seed rows of one block's last layer and their way back to the head MLP's
// output. Row r is an atom (ctr, fc null) or an edge: dY[r][p] = fc_r gA[ctr_r][p] (the cutoff factor of the atom sum, the
// centre's seed), dS[r][c] (+)= sum_p dY[r][p] W[p][c]. One launch per block, in block order: the hidden adjoint of the
// head MLP the blocks share is their sum in that fixed order.
__global__ void k_gt_last_rev(const float* __restrict__ gA, const int* __restrict__ ctr, const float* __restrict__ fc,
                              const float* __restrict__ W, int P, int DH, int64_t rows, float* __restrict__ dY,
                              float* __restrict__ dS, int acc) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * DH) return;
    const int64_t r = idx / DH;
    const int c = (int)(idx % DH);
    const int64_t i = ctr ? (int64_t)ctr[r] : r;
    const float f = fc ? fc[r] : 1.f;
    float s = 0.f;
    for (int p = 0; p < P; p++) {
        const float v = f * gA[i * P + p];
        s = fmaf(v, W[(int64_t)p * DH + c], s);
        if (dY && c == 0) dY[r * P + p] = v;
    }
    dS[idx] = acc ? dS[idx] + s : s;
}

// ---------------------------------------------------------------------------------------------
// long-range stage: the layer sum, the mix and their adjoints (one half of a dual row set per launch)
// ---------------------------------------------------------------------------------------------
constexpr int LR_MAX_LAYERS = 16;
struct LrRows {
    const float* p[LR_MAX_LAYERS];
    int n;
};
// Y = scale * sum_l X_l, the layers added in layer order by one thread per element: x = sum_l h_l / sqrt(NR) forward, and
// the adjoint of y from those of the m_l, sum_l / sqrt(2), in reverse
__global__ void k_lr_layer_sum(LrRows X, float scale, float* __restrict__ Y, int64_t n) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    float s = X.p[0][idx];
    for (int l = 1; l < X.n; l++) s += X.p[l][idx];
    Y[idx] = scale * s;
}
// m_l = (h_l + y) / sqrt(2)
__global__ void k_lr_mix(const float* __restrict__ H, const float* __restrict__ Y, float* __restrict__ M, int64_t n) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < n) M[idx] = (H[idx] + Y[idx]) * 0.70710678118654752f;
}
// the adjoint of h_l from that of m_l (in place) and that of x: dH = dM / sqrt(2) + dX * sx, sx = 1 / sqrt(NR)
__global__ void k_lr_mix_rev(float* __restrict__ dH, const float* __restrict__ dX, float sx, int64_t n) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < n) dH[idx] = fmaf(dX[idx], sx, dH[idx] * 0.70710678118654752f);
}
// nu_q = A nu_V + (D_u A) lambda_V: the second term added where there is a direction
__global__ void k_lr_add(float* __restrict__ Y, const float* __restrict__ X, int64_t n) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < n) Y[idx] += X[idx];
}

// ---------------------------------------------------------------------------------------------
// workspace of the pass
// ---------------------------------------------------------------------------------------------
using TAttn = WAttn<D2>;
using TGnn = WGnn<D2>;
struct TWs {
    std::vector<TGnn> gnn;
    D2 H0, M0, geo;
    float *fcd, *bd;
    D2 tE[5], tN[4];          // temporaries [R][wmax] / [N][nmax]
    D2 dX, dX2, dM, dH, dQKV; // adjoints
    float *CC, *DD, *part;
    size_t part_floats;
    size_t bytes;
};
static int n_chunks_for(int64_t rows) { return (int)std::min<int64_t>(32, std::max<int64_t>(1, (rows + 1023) / 1024)); }
static void train_carve(const Model& m, int64_t N, int64_t E, void* base, TWs& w) {
    const GD d = dims_of(m);
    Carver c(base);
    const int64_t R = E + N, Ra = R > 0 ? R : 1, Na = N > 0 ? N : 1, Ea = E > 0 ? E : 1;
    take(c, Na * d.DN, w.H0);
    take(c, Ea * d.D, w.M0);
    take(c, Ea * 4, w.geo);
    w.fcd = c.take<float>(Ea);
    w.bd = c.take<float>(Ea);
    carve_layers(m, d, c, Na, Ea, Ra, w.H0, w.gnn);
    const int wmax = imax(imax(3 * d.D, 2 * d.DFF), imax(2 * d.D, d.DH));
    const int nmax = imax(imax(2 * d.DNF, d.DN), imax(d.DH, d.D));
    for (auto& t : w.tE) take(c, Ra * wmax, t);
    for (auto& t : w.tN) take(c, Na * nmax, t);
    take(c, Ra * d.D, w.dX); take(c, Ra * d.D, w.dX2);
    take(c, Ea * d.D, w.dM); take(c, Na * d.DN, w.dH);
    take(c, Ra * 3 * d.D, w.dQKV);
    w.CC = c.take<float>(Ra * d.NH);
    w.DD = c.take<float>(Ra * d.NH);
    // partial sums of the largest weight gradient (and of the embedding tables)
    size_t big = (size_t)imax(4 * d.DN * d.DN, imax(2 * d.DFF * d.D, imax(4 * d.D * d.D, 3 * d.D * d.D)));
    big = std::max(big, (size_t)imax(d.DH * d.DN, d.DH * d.DH));
    big = std::max(big, (size_t)m.h.n_species * imax(d.DN, d.D));
    w.part_floats = big * 32;
    w.part = c.take<float>(w.part_floats);
    w.bytes = c.off;
}

// ---- system conditioning (conditioning.py:82-100; backend.py:543-545, :628-629): cond_s = W2 silu(W0 [emb_q ; emb_m] + b0)
// + b2 is added to the node features LEAVING every GNN layer. It does not move with the positions (no tangent), so its
// parameters see the nu-adjoint of those features only, summed over the atoms of each system.
__global__ void k_gt_cond_accum(const float* __restrict__ dH, const int* __restrict__ sys32, const int64_t* __restrict__ sys64,
                                int N, int W, float* __restrict__ dcond, int accumulate) {
    // one block per system; its atoms are a contiguous run of the non-decreasing system indices; fixed summation order
    __shared__ int range[2];
    const int s = blockIdx.x;
    if (threadIdx.x == 0) {
        auto at = [&](int i) { return sys64 ? sys64[i] : (int64_t)sys32[i]; };
        int a = 0, b = N;
        while (a < b) { const int mid = (a + b) >> 1; if (at(mid) < s) a = mid + 1; else b = mid; }
        range[0] = a; b = N;
        while (a < b) { const int mid = (a + b) >> 1; if (at(mid) < s + 1) a = mid + 1; else b = mid; }
        range[1] = a;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < W; c += blockDim.x) {
        float acc = 0.f;
        for (int i = range[0]; i < range[1]; i++) acc += dH[(size_t)i * W + c];
        dcond[(size_t)s * W + c] = accumulate ? dcond[(size_t)s * W + c] + acc : acc;
    }
}
// ONE block walks the systems in order (a handful of rows; deterministic): every thread owns whole rows / columns of the
// gradient slots it adds to, so nothing races
__global__ __launch_bounds__(256) void k_gt_cond_bwd(const int64_t* __restrict__ charge, const int64_t* __restrict__ spin,
                                                     const float* __restrict__ qe, const float* __restrict__ se,
                                                     const float* __restrict__ w0, const float* __restrict__ b0,
                                                     const float* __restrict__ w2, const float* __restrict__ dcond, int n_sys,
                                                     int max_charge, int max_spin, int DN, float* __restrict__ gq,
                                                     float* __restrict__ gm, float* __restrict__ gw0, float* __restrict__ gb0,
                                                     float* __restrict__ gw2, float* __restrict__ gb2) {
    extern __shared__ float sm[];  // x [2 DN] | a [DN] | hid [DN] | da [DN] | dc [DN]
    float *x = sm, *a = sm + 2 * DN, *hid = a + DN, *da = hid + DN, *dc = da + DN;
    for (int s = 0; s < n_sys; s++) {
        int q = (int)charge[s] + max_charge, mi = (int)spin[s] - 1;
        q = q < 0 ? 0 : (q > 2 * max_charge ? 2 * max_charge : q);
        mi = mi < 0 ? 0 : (mi > max_spin - 1 ? max_spin - 1 : mi);
        __syncthreads();
        for (int k = threadIdx.x; k < DN; k += blockDim.x) {
            x[k] = qe[(size_t)q * DN + k];
            x[DN + k] = se[(size_t)mi * DN + k];
            dc[k] = dcond[(size_t)s * DN + k];
        }
        __syncthreads();
        for (int t = threadIdx.x; t < DN; t += blockDim.x) {
            float v = b0[t];
            for (int k = 0; k < 2 * DN; k++) v = fmaf(w0[(size_t)t * 2 * DN + k], x[k], v);
            a[t] = v;
            hid[t] = v * gsig(v);
        }
        __syncthreads();
        for (int t = threadIdx.x; t < DN; t += blockDim.x) {
            float dh = 0.f;
            for (int o = 0; o < DN; o++) dh = fmaf(w2[(size_t)o * DN + t], dc[o], dh);
            const float sg = gsig(a[t]);
            da[t] = dh * sg * (1.0f + a[t] * (1.0f - sg));
        }
        __syncthreads();
        for (int t = threadIdx.x; t < DN; t += blockDim.x) {   // rows t of project.0 / project.2 and their biases
            const float dat = da[t], dct = dc[t];
            for (int k = 0; k < 2 * DN; k++) gw0[(size_t)t * 2 * DN + k] += dat * x[k];
            for (int k = 0; k < DN; k++) gw2[(size_t)t * DN + k] += dct * hid[k];
            gb0[t] += dat;
            gb2[t] += dct;
        }
        for (int k = threadIdx.x; k < 2 * DN; k += blockDim.x) {   // columns k of the two embedding rows
            float dx = 0.f;
            for (int o = 0; o < DN; o++) dx = fmaf(w0[(size_t)o * 2 * DN + k], da[o], dx);
            if (k < DN) gq[(size_t)q * DN + k] += dx;
            else gm[(size_t)mi * DN + (k - DN)] += dx;
        }
    }
}

// The dual pass of gen_walk.h: every value a (primal, tangent) pair, every adjoint (nu, lambda). In training it forms the
// parameter gradients; in Hessian-vector mode (hv) none, and the adjoints that reach the geometry are kept instead.
struct TOps {
    using V = D2;
    using CV = D2;
    const Model& m;
    const Graph& g;
    GD d;
    hipStream_t st;
    Lins lin;
    Ops o;
    TWs* w;
    std::map<const float*, float*> off;   // raw parameter storage -> its gradient slot
    int err = PET_OK;
    const HvpTaps* hv;   // Hessian-vector mode: the sweep forms no parameter gradient and never looks at a gradient slot
    int64_t N, E, R;
    Roles<D2> s;
    D2 geo;
    float *cond = nullptr, *dcond = nullptr;   // [n_systems][DN] per-system conditioning embedding and its nu-adjoint
    std::vector<D2> dHl, dMl;                  // adjoints entering the backbone from the heads, per readout layer
    TOps(const Model& m_, const Graph& g_, hipStream_t st_, TWs* w_, const HvpTaps* hv_ = nullptr)
        : m(m_), g(g_), d(dims_of(m_)), st(st_), lin{st_}, o(m_, g_, st_), w(w_), hv(hv_), N(o.N), E(o.E), R(o.R), geo(w_->geo) {
        s.normed = w->tE[0]; s.OUT = w->tE[1]; s.act = w->tE[2]; s.nNormed = w->tN[0]; s.nAct = w->tN[1];
        s.dAO = w->tE[0]; s.dOUT = w->tE[1]; s.dVG = w->tE[2]; s.re = w->tE[3]; s.dXin = w->tE[4];
        s.dH1 = w->tN[0]; s.nA = w->tN[1]; s.nB = w->tN[2]; s.nRe = w->tN[3]; s.dTOKo = w->tN[3];
        if (hv) return;
        for (const auto& kv : m.raw) {
            auto it = m.grad_off.find(kv.first);
            if (it != m.grad_off.end()) off[kv.second.first] = m.grad_flat + it->second;
        }
        // a LoRA-adapted Linear is read as W_eff: its gradient goes to the adapter's dL/dW_eff (lora.hip projects it)
        for (const auto& kv : m.lora)
            if (kv.second.w_eff) off[kv.second.w_eff] = m.lora_grad + kv.second.dw_off;
    }
    float* slot(const float* raw) {
        auto it = off.find(raw);
        if (it == off.end()) { err = PET_ERR_ARGUMENT; set_error("gen_train: a parameter has no gradient slot"); return nullptr; }
        return it->second;
    }
    // ---- forward operations
    void linf(const D2& X, int64_t ldx, const Lin& L, const D2& Y, int64_t ldy, int64_t rows, bool acc = false) const {
        if (rows <= 0) return;
        lin.fwd(X.p, ldx, L, Y.p, ldy, rows, acc);
        Lin nb = L;
        nb.b = nullptr;   // the tangent of a Linear has no bias
        lin.fwd(X.t, ldx, nb, Y.t, ldy, rows, acc);
    }
    void norm(const D2& X, const float* gamma, const float* beta, const D2& Y, int64_t rows, int W, int ln = -1, float e = -1.f) const {
        if (rows <= 0) return;
        const int l = ln < 0 ? (int)m.layer_norm() : ln;
        k_gt_norm<<<(int)cdiv(rows, 4), 256, 0, st>>>(X.p, X.t, gamma, l ? beta : nullptr, l, e < 0 ? o.eps() : e, Y.p, Y.t, rows, W);
    }
    void silu(const D2& A, const D2& S, int64_t n) const { if (n > 0) k_gt_silu<<<g1(n), 256, 0, st>>>(A.p, A.t, S.p, S.t, n); }
    void swiglu(const D2& VG, const D2& S, int64_t rows, int F) const {
        if (rows > 0) k_gt_swiglu<<<g1(rows * F), 256, 0, st>>>(VG.p, VG.t, S.p, S.t, rows, F);
    }
    void axpby(float a, const D2& A, int64_t lda, float b, const D2& B, int64_t ldb, const int* index, const D2& Y, int64_t ldy,
               bool acc, int64_t rows, int W) const {
        o.axpby(a, A.p, lda, b, B.p, ldb, index, Y.p, ldy, acc, rows, W);
        o.axpby(a, A.t, lda, b, B.t, ldb, index, Y.t, ldy, acc, rows, W);
    }
    void copy(const D2& A, const D2& Y, int64_t rows, int W) const { axpby(1.f, A, W, 0.f, D2(), 0, nullptr, Y, W, false, rows, W); }
    void zero(const D2& A, int64_t n) const { o.zero(A.p, n); o.zero(A.t, n); }
    // a table row does not move with the positions: the tangent half is zero (a strided one by the row kernel)
    void embed(const int* index, const float* table, const D2& Y, int64_t ldy, int64_t rows, int W) const {
        o.embed(index, table, Y.p, ldy, rows, W);
        if (ldy == W) o.zero(Y.t, rows * W);
        else o.axpby(0.f, nullptr, 0, 0.f, nullptr, 0, nullptr, Y.t, ldy, false, rows, W);
    }
    void attn(const TAttn& A) const {
        attn_dispatch(d.HD, [&](auto hdm) {
            k_gt_attn<decltype(hdm)::value><<<dim3((unsigned)N, (unsigned)d.NH), 64, 0, st>>>(
                A.QKV.p, A.QKV.t, g.rowptr, g.fc, w->bd, A.AO.p, A.AO.t, A.LSE, A.MS, E, d.D, d.NH, d.HD, o.scale);
        });
    }
    void add_cond(const D2& H) const { k_gen_add_cond<<<g1(N * d.DN), 256, 0, st>>>(H.p, cond, g.sys, g.cond_sys, N, d.DN); }
    void re_norm(const D2& X, const float* gamma, const float* beta, const D2& Y, int64_t rows, int W, int ln = -1, float e = -1.f) const {
        norm(X, gamma, beta, Y, rows, W, ln, e);
    }
    void re_silu(const D2& A, const D2& S, int64_t n) const { silu(A, S, n); }
    void re_swiglu(const D2& VG, const D2& S, int64_t rows, int F) const { swiglu(VG, S, rows, F); }
    // ---- reverse operations
    void chunked(int64_t rows, int& nc, int64_t& per) const {
        nc = n_chunks_for(rows);
        per = (rows + nc - 1) / nc;
    }
    // dW += nu_y^T x + lambda_y^T x', db += colsum(nu_y)
    void wgrad(const Lin& L, const D2& NY, int64_t ldy, const D2& X, int64_t ldx, int64_t rows) {
        if (rows <= 0 || err || hv) return;
        int nc; int64_t per;
        chunked(rows, nc, per);
        float* gw = slot(L.w);
        if (!gw) return;
        dim3 grid((unsigned)cdiv(L.n_out, 64), (unsigned)cdiv(L.k_in, 64), (unsigned)nc);
        k_gt_wgrad<<<grid, 256, 0, st>>>(NY.p, X.p, NY.t, X.t, ldy, ldx, rows, L.n_out, L.k_in, per, w->part);
        const int64_t n = (int64_t)L.n_out * L.k_in;
        k_gt_reduce<<<g1(n), 256, 0, st>>>(w->part, nc, n, gw);
        if (L.b) colsum(NY.p, ldy, rows, L.n_out, slot(L.b));
    }
    void colsum(const float* A, int64_t lda, int64_t rows, int W, float* dst) {
        if (rows <= 0 || !dst) return;
        int nc; int64_t per;
        chunked(rows, nc, per);
        k_gt_colsum<<<dim3((unsigned)cdiv(W, 64), (unsigned)nc), 64, 0, st>>>(A, lda, rows, W, per, w->part);
        k_gt_reduce<<<g1(W), 256, 0, st>>>(w->part, nc, W, dst);
    }
    void embed_grad(const int* index, const D2& NU, int64_t ld, int64_t rows, int W, const float* table) {   // (the nu half)
        if (rows <= 0 || err || hv) return;
        float* dst = slot(table);
        if (!dst) return;
        int nc; int64_t per;
        chunked(rows, nc, per);
        const int ns = m.h.n_species;
        k_gt_embed_grad<<<dim3((unsigned)cdiv(W, 64), (unsigned)nc), 64, 0, st>>>(index, NU.p, ld, rows, W, ns, per, w->part);
        k_gt_reduce<<<g1((int64_t)ns * W), 256, 0, st>>>(w->part, nc, (int64_t)ns * W, dst);
    }
    // (nu_x, lambda_x) (+)= W^T (nu_y, lambda_y)
    void linb(const D2& NY, int64_t ldy, const Lin& L, const D2& NX, int64_t ldx, int64_t rows, bool acc = false) const {
        if (rows <= 0) return;
        lin.bwd(NY.p, ldy, L, NX.p, ldx, rows, acc);
        lin.bwd(NY.t, ldy, L, NX.t, ldx, rows, acc);
    }
    // norm reverse incl. the norm's own parameter gradients; G: scratch [rows][W] (its primal half)
    void norm_rev(const D2& X, const float* gamma, const float* beta, const D2& NY, const D2& NX, bool acc, const D2& G, int64_t rows,
                  int W, int ln = -1, float e = -1.f) {
        if (rows <= 0) return;
        const int l = ln < 0 ? (int)m.layer_norm() : ln;
        k_gt_norm_rev<<<(int)cdiv(rows, 4), 256, 0, st>>>(X.p, X.t, gamma, l, e < 0 ? o.eps() : e, NY.p, NY.t, NX.p, NX.t, acc,
                                                          hv ? nullptr : G.p, rows, W);
        if (hv) return;
        colsum(G.p, W, rows, W, slot(gamma));
        if (l && beta) colsum(NY.p, W, rows, W, slot(beta));
    }
    void silu_rev(const D2& A, const D2& NS, int64_t n) const {   // in place on the adjoint
        if (n > 0) k_gt_silu_rev<<<g1(n), 256, 0, st>>>(A.p, A.t, NS.p, NS.t, NS.p, NS.t, n);
    }
    void swiglu_rev(const D2& VG, const D2& NS, const D2& NVG, int64_t rows, int F) const {
        if (rows > 0) k_gt_swiglu_rev<<<g1(rows * F), 256, 0, st>>>(VG.p, VG.t, NS.p, NS.t, NVG.p, NVG.t, rows, F);
    }
    void attn_rev(const TAttn& A, const D2& dAO) const {   // -> w->dQKV; hv: the key-bias adjoints per head too
        attn_dispatch(d.HD, [&](auto hdm) {
            constexpr int HDM = decltype(hdm)::value;
            const dim3 grid((unsigned)N, (unsigned)d.NH);
            k_gt_attn_rev_q<HDM><<<grid, 64, 0, st>>>(A.QKV.p, A.QKV.t, dAO.p, dAO.t, A.LSE, A.MS, g.rowptr, g.fc, w->bd, w->dQKV.p,
                                                      w->dQKV.t, w->CC, w->DD, E, d.D, d.NH, d.HD, o.scale);
            if (!hv)
                k_gt_attn_rev_k<HDM><<<grid, 64, 0, st>>>(A.QKV.p, A.QKV.t, dAO.p, dAO.t, A.LSE, A.MS, w->CC, w->DD, g.rowptr, g.fc,
                                                          w->bd, w->dQKV.p, w->dQKV.t, E, d.D, d.NH, d.HD, o.scale, nullptr, nullptr);
            else
                k_gt_attn_rev_k<HDM, true><<<grid, 64, 0, st>>>(A.QKV.p, A.QKV.t, dAO.p, dAO.t, A.LSE, A.MS, w->CC, w->DD, g.rowptr,
                                                                g.fc, w->bd, w->dQKV.p, w->dQKV.t, E, d.D, d.NH, d.HD, o.scale, hv->sb,
                                                                hv->sdb);
        });
    }
    // ---- sinks: heads in head order, attention layers and GNN layers in the order the sweep visits them
    void key_bias_sink(bool first) const {
        if (hv && E > 0) k_hvp_bias_sum<<<g1(E), 256, 0, st>>>(hv->sb, hv->sdb, d.NH, E, hv->db, hv->dbd, !first);
    }
    void geo_sink(const D2& dTOK, int kin, const Lin& eemb, bool first) const {   // (nu, lambda) of geo, over the layers
        if (hv) linb(dTOK, kin, eemb, D2{hv->ngeo, hv->lgeo}, 4, E, !first);
    }
    void cond_accum(const D2& dH, bool first) const {
        if (dcond && !hv) k_gt_cond_accum<<<(int)g.n_cond_systems, 256, 0, st>>>(dH.p, g.sys, g.cond_sys, (int)N, d.DN, dcond, !first);
    }
    void seed(int l, const D2& dH, const D2& dE) const {   // (one readout layer, no residual: the heads wrote them in place)
        if (dHl[l].p == dH.p) return;
        copy(dHl[l], dH, N, d.DN);
        copy(dMl[l], dE, E, d.D);
    }
    // reverse of one head branch (gen_head on X, then the last layer): gradients of its three Linears, the adjoint of X -> dX
    void head_rev(const Lin& last, const Lin& h2, const Lin& h0, const D2& seeds, const D2& X, int W, int64_t rows, const D2& a1,
                  const D2& s1, const D2& a2, const D2& s2, const D2& dX) {
        const int DH = d.DH;
        wgrad(last, seeds, 1, s2, DH, rows);
        linb(seeds, 1, last, s2, DH, rows);   // (nu, lambda) of s2
        silu_rev(a2, s2, rows * DH);
        wgrad(h2, s2, DH, s1, DH, rows);
        linb(s2, DH, h2, s1, DH, rows);       // of s1
        silu_rev(a1, s1, rows * DH);
        wgrad(h0, s1, DH, X, W, rows);
        linb(s1, DH, h0, dX, W, rows);
    }
};

// ---------------------------------------------------------------------------------------------
// The long-range stage (LrStage, model.h): between the backbone and the heads,
//     x = sum_l h_l / sqrt(NR),  q = C x + c,  V = A(r) q,  a = P0 V + p0,  s = silu(a),  y = P2 s + p2,  m_l = (h_l + y) / sqrt(2)
// on dual rows [N, d_node] (every Linear of the featuriser is d_node x d_node), with V' = A q' + (D_u A) q from the
// operator's second-order entry (out_grad_potential at u_q = q', u_r = u). The heads read m_l.
// ---------------------------------------------------------------------------------------------
const char* const LR_KEYS[3] = {"long_range_featurizer.charges_map", "long_range_featurizer.out_projection.0",
                                "long_range_featurizer.out_projection.2"};
struct LrWs {
    void* ew;                             // the operator's workspace (lr_workspace_bytes at d_node channels)
    LrCall op;                            // the operator's call context on it (gen_train2 fills it once per stage)
    D2 x, q, V, a, s, y, dy, dV, dq, dx;  // values and adjoints [N, d_node]
    float *dqu, *r1, *r2;                 // (D_u A) lambda_V [N, d_node]; the operator's two position adjoints [N, 3]
    std::vector<D2> ml;
    size_t bytes;
};
static void lr_carve(const Model& m, const pet_ewald_t* e, int64_t N, void* base, LrWs& w, bool cell = false) {
    const GD d = dims_of(m);
    Carver c(base);
    w.ew = base;
    c.off = ((size_t)lr_workspace_bytes(e, d.DN, cell) + 255) & ~size_t(255);
    const size_t n = (size_t)(N > 0 ? N : 1) * d.DN;
    for (D2* v : {&w.x, &w.q, &w.V, &w.a, &w.s, &w.y, &w.dy, &w.dV, &w.dq, &w.dx}) take(c, n, *v);
    w.dqu = c.take<float>(n);
    w.r1 = c.take<float>((size_t)(N > 0 ? N : 1) * 3);
    w.r2 = c.take<float>((size_t)(N > 0 ? N : 1) * 3);
    w.ml.resize(m.num_readout_layers());
    for (auto& v : w.ml) take(c, n, v);
    w.bytes = c.off;
}
// the three Linears from the model's own parameter table; a missing (or mis-sized) tensor is an error by key
static int lr_linears(const Model& m, int DN, Lin* L) {
    for (int i = 0; i < 3; i++) {
        const std::string k(LR_KEYS[i]);
        auto wi = m.raw.find(k + ".weight"), bi = m.raw.find(k + ".bias");
        PET_REQUIRE(wi != m.raw.end() && wi->second.second == (int64_t)DN * DN, PET_ERR_ARGUMENT,
                    "the model holds no '" + k + ".weight' of d_node x d_node elements: load the long-range checkpoint's "
                    "featuriser tensors with the model (HipModel.load uploads every key of a state dict)");
        PET_REQUIRE(bi != m.raw.end() && bi->second.second == (int64_t)DN, PET_ERR_ARGUMENT,
                    "the model holds no '" + k + ".bias' of d_node elements: load the long-range checkpoint's featuriser "
                    "tensors with the model (HipModel.load uploads every key of a state dict)");
        L[i] = Lin();
        L[i].w = wi->second.first;
        L[i].b = bi->second.first;
        L[i].n_out = L[i].k_in = DN;
    }
    return PET_OK;
}
static LrRows lr_rows(const std::vector<D2>& v, bool tangent) {
    LrRows r;
    r.n = (int)v.size();
    for (int l = 0; l < r.n; l++) r.p[l] = tangent ? v[l].t : v[l].p;
    return r;
}
// sweep 1: h_l (the backbone's node features per readout layer) -> m_l. Without a direction every tangent row is zero.
static int lr_forward(TOps& t, const LrStage& lr, const Lin* L, const std::vector<D2>& h, const float* u, LrWs& w) {
    const int64_t N = t.N, n = t.N * t.d.DN;
    const int DN = t.d.DN;
    const float sx = 1.0f / sqrtf((float)h.size());
    k_lr_layer_sum<<<g1(n), 256, 0, t.st>>>(lr_rows(h, false), sx, w.x.p, n);
    k_lr_layer_sum<<<g1(n), 256, 0, t.st>>>(lr_rows(h, true), sx, w.x.t, n);
    t.linf(w.x, DN, L[0], w.q, DN, N);
    PET_TRY(lr_potential(w.op, w.q.p, w.V.p));
    if (u) PET_TRY(lr_second(w.op, w.q.p, nullptr, w.q.t, u, lr.ucell, nullptr, w.V.t, nullptr));  // V' = A q' + (D A) q along (u, ucell)
    else t.o.zero(w.V.t, n);
    t.linf(w.V, DN, L[1], w.a, DN, N);
    t.silu(w.a, w.s, n);
    t.linf(w.s, DN, L[2], w.y, DN, N);
    for (size_t l = 0; l < h.size(); l++) {
        k_lr_mix<<<g1(n), 256, 0, t.st>>>(h[l].p, w.y.p, w.ml[l].p, n);
        k_lr_mix<<<g1(n), 256, 0, t.st>>>(h[l].t, w.y.t, w.ml[l].t, n);
    }
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}
// sweep 2: t.dHl holds the heads' adjoint pairs of (m_l, m_l'); on return those of (h_l, h_l'). The six gradients go to
// their slots; in Hessian-vector mode none is formed and lr.rbar receives the operator's share of dJ/dR instead:
//     grad_r Phi(r; nu_V, q) + grad_r Phi(r; q', lambda_V) + H_Phi(r; lambda_V, q) u.
static int lr_reverse(TOps& t, const LrStage& lr, const Lin* L, const float* u, LrWs& w) {
    const int64_t N = t.N, n = t.N * t.d.DN;
    const int DN = t.d.DN;
    k_lr_layer_sum<<<g1(n), 256, 0, t.st>>>(lr_rows(t.dHl, false), 0.70710678118654752f, w.dy.p, n);
    k_lr_layer_sum<<<g1(n), 256, 0, t.st>>>(lr_rows(t.dHl, true), 0.70710678118654752f, w.dy.t, n);
    t.wgrad(L[2], w.dy, DN, w.s, DN, N);
    t.linb(w.dy, DN, L[2], w.s, DN, N);     // (nu, lambda) of s, then of a
    t.silu_rev(w.a, w.s, n);
    t.wgrad(L[1], w.s, DN, w.V, DN, N);
    t.linb(w.s, DN, L[1], w.dV, DN, N);     // (nu_V, lambda_V)
    // lambda_q' = A lambda_V, nu_q = A nu_V + (D_u A) lambda_V (A and D_u A are symmetric)
    if (t.hv) {
        PET_TRY(lr_backward(w.op, w.q.p, w.dV.p, w.dq.p, w.r1));
        PET_TRY(lr_second(w.op, w.q.p, w.dV.t, w.q.t, u, nullptr, w.dqu, nullptr, w.r2));
        t.o.axpby(1.f, w.r1, 3, 1.f, w.r2, 3, nullptr, lr.rbar, 3, false, N, 3);
    } else {
        PET_TRY(lr_potential(w.op, w.dV.p, w.dq.p));
        if (u) PET_TRY(lr_second(w.op, nullptr, w.dV.t, nullptr, u, lr.ucell, w.dqu, nullptr, nullptr));
    }
    if (u) {
        PET_TRY(lr_potential(w.op, w.dV.t, w.dq.t));
        k_lr_add<<<g1(n), 256, 0, t.st>>>(w.dq.p, w.dqu, n);
    } else
        t.o.zero(w.dq.t, n);
    t.wgrad(L[0], w.dq, DN, w.x, DN, N);
    t.linb(w.dq, DN, L[0], w.dx, DN, N);
    const float sx = 1.0f / sqrtf((float)t.dHl.size());
    for (auto& dh : t.dHl) {
        k_lr_mix_rev<<<g1(n), 256, 0, t.st>>>(dh.p, w.dx.p, sx, n);
        k_lr_mix_rev<<<g1(n), 256, 0, t.st>>>(dh.t, w.dx.t, sx, n);
    }
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

}  // namespace

// (nu_x, lambda_x) = adjoint of (y, y') = norm(x, x') on rows of any width (k_gt_norm_rev) for another caller: the
// SOAP-BPNN training pass of legacy = False models takes its LayerNorm adjoints here (soap_train.hip)
int norm_rev_rows(const float* Xp, const float* Xt, const float* gamma, int ln, float eps, const float* NYp, const float* NYt,
                  float* NXp, float* NXt, int64_t R, int W, hipStream_t st) {
    if (R <= 0) return PET_OK;
    k_gt_norm_rev<<<(int)cdiv(R, 4), 256, 0, st>>>(Xp, Xt, gamma, ln, eps, NYp, NYt, NXp, NXt, 0, nullptr, R, W);
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

int64_t gen_train_workspace_bytes(const Model& m, int64_t N, int64_t E) {
    TWs w;
    train_carve(m, N, E, nullptr, w);
    return (int64_t)w.bytes;
}

// dL/d theta of J = sum_i (nu_i e_i + lambda_i e'_i) ADDED to the flat gradient; tangent_atomic [N] = e'_i (optional).
// nA / lA may be null (zero). u null = no tangent (energy-only loss).
// seed_node / seed_edge [n_seed] (NULL entries = 0): feature adjoints of further targets (gen_train_predict_backward), one
// pair per readout layer, added to the nu half where the fused head's adjoint enters the backbone (first-order terms: the
// lambda half is theirs no more than a tangent is). lA and nA both null: no fused target in the loss, its heads are
// neither needed nor touched.
// hv (gen_hvp below): Hessian-vector mode. No parameter gradient is formed and no gradient slot is touched; sweep 2 instead
// keeps the adjoints that reach the geometry -- of geo = (v, d), of the key bias and of the cutoff factor, each a
// (nu, lambda) pair -- and k_hvp_geo folds them into hv->dv = dJ/dv [E, 4]. Needs u and a static cutoff.
int gen_train2(const Model& m, const Graph& g, void* ws2, int64_t ws2_bytes, const float* lA, const float* nA, const float* u,
               const float* ucell, float* tangent_atomic, hipStream_t st, const float* const* seed_node,
               const float* const* seed_edge, int n_seed, const HvpTaps* hv, const LrStage* lr) {
    PET_REQUIRE(!lr || ((lA || nA) && (!ucell || (lr->ucell && !hv)) && n_seed == 0 && !g.adaptive), PET_ERR_ARGUMENT,
                "the long-range stage: the fused target's seeds, no cell tangent (but pet_backward_train2_long_range_cell's), no "
                "seeds of further targets, a static cutoff");
    PET_REQUIRE(!lr || !lr->ucell || lr->ucell == ucell, PET_ERR_ARGUMENT,
                "the long-range stage and the backbone take one cell tangent: LrStage::ucell is gen_train2's ucell");
    PET_REQUIRE(hv || m.grad_flat, PET_ERR_ARGUMENT, "pet_model_zero_grad has not been called");
    PET_REQUIRE(!hv || (u && !g.adaptive && n_seed == 0), PET_ERR_ARGUMENT, "Hessian-vector mode: a direction, a static cutoff, no seeds");
    PET_REQUIRE(n_seed == 0 || n_seed == m.num_readout_layers(), PET_ERR_ARGUMENT, "expected one seed pair per readout layer");
    const bool fused = lA || nA;
    if (!fused) {
        if (tangent_atomic && g.n_nodes > 0) PET_HIP_CHECK(hipMemsetAsync(tangent_atomic, 0, g.n_nodes * sizeof(float), st));
        bool seeded = false;
        for (int l = 0; l < n_seed; l++) seeded = seeded || (seed_node && seed_node[l]) || (seed_edge && seed_edge[l]);
        if (!seeded || !backbone_trainable(m)) return PET_OK;  // nothing enters the backbone / only heads and last layers train
    }
    const bool conditioned = m.h.system_conditioning != 0;
    if (conditioned)
        PET_REQUIRE(g.cond_charge && g.n_cond_systems >= 1 && g.n_cond_systems <= g.n_nodes, PET_ERR_ARGUMENT,
                    "system_conditioning: call pet_graph_set_conditioning (charge, spin multiplicity, system indices) first");
    TWs w;
    train_carve(m, g.n_nodes, g.n_edges, ws2, w);
    PET_REQUIRE((int64_t)w.bytes <= ws2_bytes, PET_ERR_ARGUMENT, "second-order workspace too small");
    TOps t(m, g, st, &w, hv);
    const GD& d = t.d;
    const int64_t N = t.N, E = t.E, R = t.R;
    if (N == 0) return PET_OK;
    const int D = d.D, DN = d.DN, DH = d.DH, NR = m.num_readout_layers();
    const bool res = m.residual();
    // the heads of the trained target, one per readout layer
    std::vector<const HeadW*> heads(NR);
    std::vector<const LastW*> lasts(NR);
    for (int l = 0; fused && l < NR; l++) {
        int rc = fused_heads(m, l, heads[l], lasts[l],
                             "training needs the single-property target uploaded as the fused head of every readout layer");
        if (rc) return rc;
    }
    PoolBuf cond_pool, extra_pool;   // returned to the stream's pool on every exit
    if (conditioned) {
        const size_t nc = (size_t)g.n_cond_systems * DN;
        PET_HIP_CHECK(cond_pool.alloc(2 * nc * sizeof(float), st));
        t.cond = cond_pool.as<float>();
        t.dcond = t.cond + nc;
        k_gen_system_cond<<<(int)g.n_cond_systems, 128, 3 * DN * sizeof(float), st>>>(
            g.cond_charge, g.cond_spin, m.cond_qe, m.cond_se, m.cond_w0, m.cond_b0, m.cond_w2, m.cond_b2, t.cond, m.h.max_charge,
            DN);
    }
    // ---------------- sweep 1: dual forward ----------------
    // geometry: primal = the graph's geo / fc, tangent along (u, ucell)
    PET_HIP_CHECK(hipMemcpyAsync(w.geo.p, g.geo, E * 4 * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (u) {
        PET_REQUIRE(!ucell || g.shift, PET_ERR_ARGUMENT, "a cell tangent needs a pet_graph_build handle (cell shifts)");
        if (E > 0 && g.adaptive) {   // the pair cutoffs move with the positions too (so.hip: implicit-function tangent of the solver)
            int rc = geometry_tangent(m, g, u, ucell, w.geo.t, w.fcd, w.bd, st);
            if (rc) return rc;
        } else if (E > 0)
            k_gt_geo<<<g1(E), 256, 0, st>>>(g.geo, g.d0, g.fc, g.ctr, g.nbr, g.shift, g.sys, u, ucell,
                                            reinterpret_cast<float4*>(w.geo.t), w.fcd, w.bd, E, m.h.cutoff, m.h.cutoff_width,
                                            m.h.cutoff_function);
    } else {
        PET_HIP_CHECK(hipMemsetAsync(w.geo.t, 0, E * 4 * sizeof(float), st));
        PET_HIP_CHECK(hipMemsetAsync(w.fcd, 0, E * sizeof(float), st));
        PET_HIP_CHECK(hipMemsetAsync(w.bd, 0, E * sizeof(float), st));
    }
    gen_walk_forward(t, w);
    // ---------------- the long-range stage, forward: the heads' node inputs become m_l ----------------
    LrWs lw;
    Lin lrl[3];
    if (lr) {
        PET_REQUIRE(NR <= LR_MAX_LAYERS, PET_ERR_UNSUPPORTED, "the long-range stage serves at most 16 readout layers");
        if (int rc = lr_linears(m, DN, lrl)) return rc;
        lr_carve(m, lr->e, N, lr->ws, lw, lr->ucell != nullptr);
        PET_REQUIRE((int64_t)lw.bytes <= lr->ws_bytes, PET_ERR_ARGUMENT, "long-range stage workspace too small");
        lw.op = LrCall{lr->e, &g, lr->pos, DN, lw.ew, lr->ws_offset, st};
        std::vector<D2> hl(NR);
        for (int l = 0; l < NR; l++) hl[l] = (res ? w.gnn[l] : w.gnn.back()).Hout;
        if (int rc = lr_forward(t, *lr, lrl, hl, u, lw)) return rc;
    }
    // ---------------- heads: tangent energies and the seeds of sweep 2 ----------------
    // adjoints entering the backbone from the heads, per readout layer: kept apart for the residual featuriser
    t.dHl.resize(NR);
    t.dMl.resize(NR);
    {
        size_t fl = 0;
        if (NR > 1 || res) fl = (size_t)NR * 2 * ((size_t)N * DN + (size_t)E * D);   // (residual, one layer: dM is zeroed by the walk)
        fl += 2 * (size_t)(N + E) + 4 * (size_t)(N + E);   // predictions (dual) and their adjoints
        PET_HIP_CHECK(extra_pool.alloc(fl * sizeof(float), st));
    }
    float* ex = extra_pool.as<float>();
    D2 npred{ex, ex + N}; ex += 2 * N;
    D2 epred{ex, ex + E}; ex += 2 * E;
    D2 nnp{ex, ex + N}; ex += 2 * N;
    D2 nep{ex, ex + E}; ex += 2 * E;
    for (int l = 0; l < NR; l++) {
        if (NR > 1 || res) {
            t.dHl[l] = D2{ex, ex + N * DN}; ex += 2 * N * DN;
            t.dMl[l] = D2{ex, ex + E * D}; ex += 2 * E * D;
        } else { t.dHl[l] = w.dH; t.dMl[l] = w.dM; }
    }
    if (fused) k_gt_seeds<<<g1(R), 256, 0, st>>>(nA, lA, g.ctr, g.fc, w.fcd, nnp.p, nnp.t, nep.p, nep.t, N, E);
    for (int l = 0; !fused && l < NR; l++) {   // no fused head: the further targets' seeds are all that enters
        t.zero(t.dHl[l], N * DN);
        t.zero(t.dMl[l], E * D);
    }
    for (int l = 0; fused && l < NR; l++) {
        const TGnn& Bl = res ? w.gnn[l] : w.gnn.back();
        const D2 Hf = lr ? lw.ml[l] : Bl.Hout, Mf = res ? Bl.XF : Bl.Mout;
        const HeadW& H = *heads[l];
        const LastW& Lw = *lasts[l];
        Lin ln; ln.w = Lw.nw; ln.b = Lw.nb; ln.n_out = 1; ln.k_in = DH;
        Lin le; le.w = Lw.ew; le.b = Lw.eb; le.n_out = 1; le.k_in = DH;
        // both branches forward (dual; the intermediates stay in the temporaries), then in reverse with weight gradients
        gen_head(t, H.nh0, H.nh2, Hf, DN, N, w.tN[0], w.tN[1], w.tN[2], w.tN[3]);
        t.linf(w.tN[3], DH, ln, npred, 1, N);
        gen_head(t, H.eh0, H.eh2, Mf, D, E, w.tE[0], w.tE[1], w.tE[2], w.tE[3]);
        t.linf(w.tE[3], DH, le, epred, 1, E);
        if (tangent_atomic)
            k_gt_atom_sum<<<g1(N), 256, 0, st>>>(npred.p, npred.t, epred.p, epred.t, g.fc, w.fcd, g.rowptr, tangent_atomic,
                                                 l > 0, N);
        if (hv && E > 0) k_hvp_fc_adj<<<g1(E), 256, 0, st>>>(nA, lA, g.ctr, epred.p, epred.t, hv->dfc, hv->dfcd, l > 0, E);
        t.head_rev(ln, H.nh2, H.nh0, nnp, Hf, DN, N, w.tN[0], w.tN[1], w.tN[2], w.tN[3], t.dHl[l]);
        t.head_rev(le, H.eh2, H.eh0, nep, Mf, D, E, w.tE[0], w.tE[1], w.tE[2], w.tE[3], t.dMl[l]);
    }
    for (int l = 0; l < n_seed; l++) {
        if (seed_node && seed_node[l]) t.o.axpby(1.f, seed_node[l], DN, 0.f, nullptr, 0, nullptr, t.dHl[l].p, DN, true, N, DN);
        if (seed_edge && seed_edge[l]) t.o.axpby(1.f, seed_edge[l], D, 0.f, nullptr, 0, nullptr, t.dMl[l].p, D, true, E, D);
    }
    // ---------------- the long-range stage, reverse: the adjoints of m_l become those of h_l ----------------
    if (lr)
        if (int rc = lr_reverse(t, *lr, lrl, u, lw)) return rc;
    // ---------------- sweep 2: joint reverse through the backbone ----------------
    gen_walk_reverse(t, w);
    if (conditioned && !hv) {
        float *gq = t.slot(m.cond_qe), *gm = t.slot(m.cond_se), *gw0 = t.slot(m.cond_w0), *gb0 = t.slot(m.cond_b0),
              *gw2 = t.slot(m.cond_w2), *gb2 = t.slot(m.cond_b2);
        if (!t.err)
            k_gt_cond_bwd<<<1, 256, 6 * DN * sizeof(float), st>>>(g.cond_charge, g.cond_spin, m.cond_qe, m.cond_se, m.cond_w0,
                                                                  m.cond_b0, m.cond_w2, t.dcond, (int)g.n_cond_systems,
                                                                  m.h.max_charge, m.h.max_spin_multiplicity, DN, gq, gm, gw0,
                                                                  gb0, gw2, gb2);
    }
    if (hv && E > 0)
        k_hvp_geo<<<g1(E), 256, 0, st>>>(g.geo, reinterpret_cast<const float4*>(w.geo.t), g.d0, g.fc, w.fcd,
                                         reinterpret_cast<const float4*>(hv->ngeo), reinterpret_cast<const float4*>(hv->lgeo),
                                         hv->db, hv->dbd, hv->dfc, hv->dfcd, reinterpret_cast<float4*>(hv->dv), E, m.h.cutoff,
                                         m.h.cutoff_width, m.h.cutoff_function);
    PET_HIP_CHECK(hipGetLastError());
    return t.err;
}

// ---------------------------------------------------------------------------------------------
// Hessian-vector product of the fused single-property target (pet_hessian_vector)
// ---------------------------------------------------------------------------------------------
namespace {
__global__ void k_hvp_fill(float* __restrict__ x, float v, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] = v;
}
// the taps and the unit weights, carved behind the dual activations of the training pass
static size_t hvp_carve(const Model& m, int64_t N, int64_t E, void* base, size_t train_bytes, HvpTaps& h, float** ones) {
    Carver c(base);
    c.off = train_bytes;
    const size_t Ea = E > 0 ? E : 1, Na = N > 0 ? N : 1;
    h.ngeo = c.take<float>(4 * Ea); h.lgeo = c.take<float>(4 * Ea);
    h.sb = c.take<float>(Ea * m.h.num_heads); h.sdb = c.take<float>(Ea * m.h.num_heads);
    h.db = c.take<float>(Ea); h.dbd = c.take<float>(Ea);
    h.dfc = c.take<float>(Ea); h.dfcd = c.take<float>(Ea);
    h.dv = c.take<float>(4 * Ea);
    *ones = c.take<float>(Na);
    return c.off;
}
}  // namespace

int64_t gen_hvp_workspace_bytes(const Model& m, int64_t N, int64_t E) {
    HvpTaps h;
    float* ones;
    return (int64_t)hvp_carve(m, N, E, nullptr, (size_t)gen_train_workspace_bytes(m, N, E), h, &ones);
}

// hvp_pos [N, 3] (and hvp_cell [S, 3, 3]) = grad_R (grad_cell) of sum_i lambda_i e'_i, e'_i = d/d eps e_i(R + eps u,
// cell + eps ucell): gen_train2 with nu = 0 in Hessian-vector mode, then the scatter of the first-order geometry adjoint.
int gen_hvp(const Model& m, const Graph& g, void* ws, int64_t ws_bytes, const float* lA, const float* u, const float* ucell,
            float* hvp_pos, float* hvp_cell, float* tangent_atomic, hipStream_t st) {
    const int64_t N = g.n_nodes, E = g.n_edges;
    if (hvp_cell && g.n_systems > 0) PET_HIP_CHECK(hipMemsetAsync(hvp_cell, 0, g.n_systems * 9 * sizeof(float), st));
    if (N == 0) return PET_OK;
    if (E == 0) {   // isolated atoms: nothing moves with the positions
        PET_HIP_CHECK(hipMemsetAsync(hvp_pos, 0, N * 3 * sizeof(float), st));
        if (tangent_atomic) PET_HIP_CHECK(hipMemsetAsync(tangent_atomic, 0, N * sizeof(float), st));
        return PET_OK;
    }
    HvpTaps h;
    float* ones;
    const size_t train_bytes = (size_t)gen_train_workspace_bytes(m, N, E);
    const size_t need = hvp_carve(m, N, E, ws, train_bytes, h, &ones);
    PET_REQUIRE((int64_t)need <= ws_bytes, PET_ERR_ARGUMENT, "Hessian-vector workspace too small");
    if (!lA) {
        k_hvp_fill<<<g1(N), 256, 0, st>>>(ones, 1.f, N);
        lA = ones;
    }
    int rc = gen_train2(m, g, ws, (int64_t)train_bytes, lA, nullptr, u, ucell, tangent_atomic, st, nullptr, nullptr, 0, &h);
    if (rc) return rc;
    // (h.ngeo is spent: it serves as the scatter's d/d(edge vector) scratch)
    return backward_geometry_generic(m, g, h.ngeo, h.dv, nullptr, nullptr, hvp_pos, hvp_cell, st);
}

// ---------------------------------------------------------------------------------------------
// The long-range forms (pet_backward_train2_long_range, pet_hessian_vector_long_range): ONE workspace, the dual pass'
// (and the Hessian-vector taps) first, the stage's behind. No edge-free exit: open systems interact through the operator
// beyond the cutoff, so a batch without an edge still has forces, a Hessian and featuriser gradients.
// ---------------------------------------------------------------------------------------------
static size_t align256(size_t n) { return (n + 255) & ~size_t(255); }

// The one layout of the three forms' workspace, for the size query and the runs alike: [pass | block | stage].
//   pass   the dual pass' workspace (gen_train_workspace_bytes; LR_HVP: with the Hessian-vector taps behind it)
//   block  one [N, 3] block: LR_TRAIN_CELL the zero direction of a call that has ucell alone (the backbone's geometry tangent and
//          the operator read one direction, not a null), LR_HVP rbar; LR_TRAIN has none
//   stage  the long-range stage's (lr_carve), LR_TRAIN_CELL with the operator's cell workspace in front
struct LrLayout {
    size_t train;               // gen_train_workspace_bytes, unaligned (what hvp_carve continues from)
    size_t block, stage, total; // byte offsets of the block and of the stage; the whole
};
static LrLayout lr_layout(const Model& m, const pet_ewald_t* e, int64_t N, int64_t E, LrSweep form) {
    LrLayout l;
    l.train = (size_t)gen_train_workspace_bytes(m, N, E);
    l.block = align256(form == LR_HVP ? (size_t)gen_hvp_workspace_bytes(m, N, E) : l.train);
    l.stage = l.block + (form == LR_TRAIN ? 0 : align256((size_t)(N > 0 ? N : 1) * 3 * sizeof(float)));
    LrWs w;
    lr_carve(m, e, N, nullptr, w, form == LR_TRAIN_CELL);
    l.total = l.stage + w.bytes;
    return l;
}

int64_t lr_sweep_workspace_bytes(const Model& m, const pet_ewald_t* e, int64_t N, int64_t E, LrSweep form) {
    return (int64_t)lr_layout(m, e, N, E, form).total;
}

int gen_train2_lr(const Model& m, const Graph& g, const pet_ewald_t* e, const float* pos, void* ws, int64_t ws_bytes,
                  const float* lA, const float* nA, const float* u, const float* ucell, float* tangent_atomic, hipStream_t st) {
    const int64_t N = g.n_nodes, E = g.n_edges;
    const LrLayout l = lr_layout(m, e, N, E, ucell ? LR_TRAIN_CELL : LR_TRAIN);
    PET_REQUIRE((int64_t)l.total <= ws_bytes, PET_ERR_ARGUMENT,
                std::string("workspace too small (pet_train2_long_range_") + (ucell ? "cell_" : "") + "workspace_bytes)");
    char* base = static_cast<char*>(ws);
    if (ucell && !u) {
        float* zeros = reinterpret_cast<float*>(base + l.block);
        PET_HIP_CHECK(hipMemsetAsync(zeros, 0, (size_t)(N > 0 ? N : 1) * 3 * sizeof(float), st));
        u = zeros;
    }
    LrStage lr{e, pos, base + l.stage, (int64_t)(l.total - l.stage), nullptr, (int64_t)l.stage, ucell};
    return gen_train2(m, g, ws, (int64_t)l.block, lA, nA, u, ucell, tangent_atomic, st, nullptr, nullptr, 0, nullptr, &lr);
}

// hvp_pos [N, 3] = grad_R of sum_i lambda_i e'_i of the long-range model: the backbone's share through the scatter of the
// geometry adjoint (none without an edge), the operator's own from the stage
int gen_hvp_lr(const Model& m, const Graph& g, const pet_ewald_t* e, const float* pos, void* ws, int64_t ws_bytes,
               const float* lA, const float* u, float* hvp_pos, float* tangent_atomic, hipStream_t st) {
    const int64_t N = g.n_nodes, E = g.n_edges;
    if (N == 0) return PET_OK;
    HvpTaps h;
    float* ones;
    const LrLayout l = lr_layout(m, e, N, E, LR_HVP);
    PET_REQUIRE((int64_t)l.total <= ws_bytes, PET_ERR_ARGUMENT, "workspace too small (pet_hvp_long_range_workspace_bytes)");
    hvp_carve(m, N, E, ws, l.train, h, &ones);
    float* rbar = reinterpret_cast<float*>(static_cast<char*>(ws) + l.block);
    LrStage lr{e, pos, static_cast<char*>(ws) + l.stage, (int64_t)(l.total - l.stage), rbar, (int64_t)l.stage};
    if (!lA) {
        k_hvp_fill<<<g1(N), 256, 0, st>>>(ones, 1.f, N);
        lA = ones;
    }
    int rc = gen_train2(m, g, ws, (int64_t)l.train, lA, nullptr, u, nullptr, tangent_atomic, st, nullptr, nullptr, 0, &h, &lr);
    if (rc) return rc;
    if (E > 0) {
        // (h.ngeo is spent: it serves as the scatter's d/d(edge vector) scratch)
        if ((rc = backward_geometry_generic(m, g, h.ngeo, h.dv, nullptr, nullptr, hvp_pos, nullptr, st))) return rc;
    } else
        PET_HIP_CHECK(hipMemsetAsync(hvp_pos, 0, (size_t)N * 3 * sizeof(float), st));
    k_lr_add<<<g1(N * 3), 256, 0, st>>>(hvp_pos, rbar, N * 3);
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

// Adjoint of gen_train_predict for `n_blocks` blocks of one (target, readout layer), seeds gA[b] [N, P_b]: dL/dtheta of the
// blocks' last layers and of the two head MLPs ADDED to the gradient slots (through TOps' pointer-to-slot map: a LoRA-adapted
// Linear receives dL/dW_eff, a frozen parameter's slot is cleared at the exit of the step's reverse entry point like every
// other slot of this pass), the adjoints of the heads' inputs ADDED to seed_node [N, d_node] / seed_edge [E, d_pet] (either
// may be null). The head MLPs run once: their hidden adjoint is the sum over the blocks in block order (k_gt_last_rev).
// First order: the weight-gradient reductions run without a tangent half. Features are read from the FORWARD workspace.
int gen_train_predict_backward(const Model& m, const Graph& g, void* ws, int64_t ws_bytes, int layer, const HeadW& H,
                               int n_blocks, const LastW* const* Lw, const float* const* gA, float* seed_node,
                               float* seed_edge, hipStream_t st) {
    PET_REQUIRE(m.grad_flat, PET_ERR_ARGUMENT, "pet_model_zero_grad has not been called");
    PET_REQUIRE(layer >= 0 && layer < m.num_readout_layers(), PET_ERR_ARGUMENT, "readout layer out of range");
    GWs f;
    gen_carve(m, g.n_nodes, g.n_edges, ws, f);
    PET_REQUIRE((int64_t)f.bytes <= ws_bytes, PET_ERR_ARGUMENT, "workspace too small for training");
    const int64_t N = g.n_nodes, E = g.n_edges, M = N > E ? N : E;
    if (N == 0 || n_blocks == 0) return PET_OK;
    const GD d = dims_of(m);
    const int DH = d.DH;
    int pmax = 1;
    for (int b = 0; b < n_blocks; b++) pmax = imax(pmax, Lw[b]->P);
    // a1, s1, a2, s2, ds [rows][DH] | dY [E][P] | partial sums of the largest weight gradient (32 row chunks at most)
    TWs w;
    w.part_floats = (size_t)32 * DH * imax(imax(d.DN, d.D), imax(DH, pmax));
    PoolBuf pool;
    PET_HIP_CHECK(pool.alloc(((size_t)5 * M * DH + (size_t)(E > 0 ? E : 1) * pmax + w.part_floats) * sizeof(float), st));
    float* a1 = pool.as<float>();
    float* s1 = a1 + M * DH;
    float* a2 = s1 + M * DH;
    float* s2 = a2 + M * DH;
    float* ds = s2 + M * DH;
    float* dY = ds + M * DH;
    w.part = dY + (size_t)(E > 0 ? E : 1) * pmax;
    TOps t(m, g, st, &w);
    auto half = [](const float* p) { return D2{const_cast<float*>(p), nullptr}; };   // first order: no tangent half
    auto branch = [&](bool edge, const Lin& h0, const Lin& h2, const float* X, int W, int64_t rows, float* seed) {
        if (rows <= 0) return;
        t.lin.fwd(X, W, h0, a1, DH, rows);
        k_gen_silu<<<g1(rows * DH), 256, 0, st>>>(a1, s1, rows * DH);
        t.lin.fwd(s1, DH, h2, a2, DH, rows);
        k_gen_silu<<<g1(rows * DH), 256, 0, st>>>(a2, s2, rows * DH);
        for (int b = 0; b < n_blocks; b++) {
            Lin ll;
            ll.w = edge ? Lw[b]->ew : Lw[b]->nw;
            ll.b = edge ? Lw[b]->eb : Lw[b]->nb;
            ll.n_out = Lw[b]->P;
            ll.k_in = DH;
            k_gt_last_rev<<<g1(rows * DH), 256, 0, st>>>(gA[b], edge ? g.ctr : nullptr, edge ? g.fc : nullptr, ll.w, ll.n_out, DH,
                                                        rows, edge ? dY : nullptr, ds, b > 0);
            t.wgrad(ll, half(edge ? dY : gA[b]), ll.n_out, half(s2), DH, rows);
        }
        k_gen_silu_bwd<<<g1(rows * DH), 256, 0, st>>>(a2, ds, ds, rows * DH);                  // d a2
        t.wgrad(h2, half(ds), DH, half(s1), DH, rows);
        t.lin.bwd(ds, DH, h2, s2, DH, rows);                                                    // d s1
        k_gen_silu_bwd<<<g1(rows * DH), 256, 0, st>>>(a1, s2, s2, rows * DH);                  // d a1
        t.wgrad(h0, half(s2), DH, half(X), W, rows);
        if (seed) t.lin.bwd(s2, DH, h0, seed, W, rows, true);
    };
    const bool res = m.residual();
    const GGnn& Bl = res ? f.gnn[layer] : f.gnn.back();
    branch(false, H.nh0, H.nh2, Bl.Hout, d.DN, N, seed_node);
    branch(true, H.eh0, H.eh2, res ? Bl.XF : Bl.Mout, d.D, E, seed_edge);
    PET_HIP_CHECK(hipGetLastError());
    return t.err;
}

}  // namespace pet
