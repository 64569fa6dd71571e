// Per-ray device code of the volumetric renderer, one wavefront per ray (see ray_ops.hip for the launchable kernels and
// render_fused.hip for the one-launch inference kernel that calls the same functions):
//   coarse_depth        run_nerf.py:357-379   (z_vals: linspace / lindisp / stratified jitter)
//   composite_ray       run_nerf.py:262-305   (raw2outputs) and its adjoint
//   distortion_ray      the distortion loss of a ray's compositing weights and its adjoint (not in the reference)
//   interlevel_ray      the interlevel loss of a ray's proposal weights against a target histogram and its adjoint (not in the reference)
//   sample_fine_ray     run_nerf.py:392-396,412 + run_nerf_helpers.py:196-239 (sample_pdf, sort, z_std)
// Sync: how the lanes of the ray's wavefront order their LDS traffic -- BlockSync when the wavefront is the whole workgroup
// (__syncthreads), WaveSync when other wavefronts of the workgroup work on other rays (LDS operations of one wavefront
// execute in order; only the compiler has to be held to the program order).
#pragma once
#include <hip/hip_runtime.h>
#include "nerf_common.h"
#include "launchers.h"

namespace nerf {

struct BlockSync { __device__ static __forceinline__ void sync() { __syncthreads(); } };
struct WaveSync {
    __device__ static __forceinline__ void sync() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
};

// torch.linspace(0, 1, n)[i] as ATen evaluates it: start + step * i for the first half, end - step * (n - 1 - i) for the second,
// each ONE fused multiply-add (checked against torch for n = 37 .. 192, tests/test_gpu_round3.py)
__device__ __forceinline__ float linspace01_at(int i, int n) {
    if (n == 1) return 0.0f;
    const float step = (1.0f - 0.0f) / (float)(n - 1);
    return i < n / 2 ? fmaf(step, (float)i, 0.0f) : fmaf(-step, (float)(n - 1 - i), 1.0f);
}

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------ wave scans
__device__ inline float wave_incl_scan_mul(float v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const float t = __shfl_up(v, d); if (lane >= d) v *= t; }
    return v;
}
__device__ inline float wave_incl_scan_add(float v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const float t = __shfl_up(v, d); if (lane >= d) v += t; }
    return v;
}
// inclusive suffix sum (lane i gets sum over lanes >= i): direct, no total-minus-prefix cancellation
__device__ inline float wave_incl_scan_add_rev(float v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const float t = __shfl_down(v, d); if (lane + d < 64) v += t; }
    return v;
}
__device__ inline float wave_sum(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// ------------------------------------------------------------------ coarse depths
__device__ inline float z_at(float near, float far, float t, int lindisp) {
    if (!lindisp) return near * (1.0f - t) + far * t;
    return 1.0f / (1.0f / near * (1.0f - t) + 1.0f / far * t);
}

// depth j of a ray (near, far): t(j) = t_vals[j] (or linspace01_at when t_vals is null); jittered inside its stratum when
// t_rand points at the ray's draws
template <typename T>
__device__ __forceinline__ float coarse_depth(float near, float far, T tv, int j, int S, int lindisp, const float* t_rand_row) {
    const float zj = z_at(near, far, tv(j), lindisp);
    if (!t_rand_row) return zj;
    const float z_last = z_at(near, far, tv(S - 1), lindisp);
    const float z_first = z_at(near, far, tv(0), lindisp);
    float upper, lower;
    if (j < S - 1) upper = 0.5f * (z_at(near, far, tv(j + 1), lindisp) + zj); else upper = z_last;
    if (j > 0) lower = 0.5f * (zj + z_at(near, far, tv(j - 1), lindisp)); else lower = z_first;
    return lower + (upper - lower) * t_rand_row[j];
}

// ------------------------------------------------------------------ compositing
__device__ inline float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// LDS per ray: 2*S floats (fwd) / 4*S floats (bwd); each lane touches only its own segment: no synchronisation
template <bool BWD>
__device__ __forceinline__ void composite_ray(const CompositeArgs& a, int ray, int lane, float* sm) {
    const int S = a.S;
    const int C = (S + 63) >> 6;
    const int lo = lane * C, hi = min(lo + C, S);
    const float* raw = a.raw + (size_t)ray * S * 4;
    const float* z = a.z + (size_t)ray * S;
    const float* dp = a.dirs + (size_t)ray * a.dir_stride;
    const float dn = sqrtf(dp[0] * dp[0] + dp[1] * dp[1] + dp[2] * dp[2]);
    float* s_alpha = sm;            // alpha_i
    float* s_t = sm + S;            // 1 - alpha_i + 1e-10
    float* s_e = sm + 2 * S;        // exp(-relu(sigma) * dist)        (bwd)
    float* s_gw = sm + 3 * S;       // g_i * w_i                       (bwd)

    // pass 1: opacity per sample, segment product of (1 - alpha + 1e-10)
    float seg = 1.0f;
    for (int i = lo; i < hi; ++i) {
        float dist = (i + 1 < S) ? (z[i + 1] - z[i]) : 1e10f;
        dist = dist * dn;
        float sg = raw[4 * i + 3];
        if (a.noise) sg = sg + a.noise[(size_t)ray * S + i] * a.noise_std;
        const float ex = expf(-fmaxf(sg, 0.0f) * dist);
        const float al = 1.0f - ex;
        const float t = 1.0f - al + 1e-10f;
        s_alpha[i] = al;
        s_t[i] = t;
        if (BWD) s_e[i] = (sg > 0.0f) ? ex * dist : 0.0f;      // d alpha / d sigma
        seg *= t;
    }
    const float incl = wave_incl_scan_mul(seg, lane);
    float T = __shfl_up(incl, 1);
    if (lane == 0) T = 1.0f;

    // pass 2: weights and ray integrals
    float r0 = 0.f, r1 = 0.f, r2 = 0.f, dsum = 0.f, asum = 0.f;
    const float Tstart = T;
    for (int i = lo; i < hi; ++i) {
        const float w = s_alpha[i] * T;
        T *= s_t[i];
        const float c0 = sigmoidf_(raw[4 * i]), c1 = sigmoidf_(raw[4 * i + 1]), c2 = sigmoidf_(raw[4 * i + 2]);
        r0 += w * c0; r1 += w * c1; r2 += w * c2;
        dsum += w * z[i];
        asum += w;
        if (!BWD && a.weights) a.weights[(size_t)ray * S + i] = w;
    }
    r0 = wave_sum(r0); r1 = wave_sum(r1); r2 = wave_sum(r2);
    dsum = wave_sum(dsum); asum = wave_sum(asum);
    const float ratio = dsum / asum;
    // torch.max(1e-10, ratio) propagates NaN (0/0 on empty rays): reference quirk, kept
    const float m = (ratio != ratio) ? ratio : fmaxf(1e-10f, ratio);

    if (!BWD) {
        if (lane == 0) {
            float w0 = r0, w1 = r1, w2 = r2;
            if (a.white_bkgd) { const float bg = 1.0f - asum; w0 = w0 + bg; w1 = w1 + bg; w2 = w2 + bg; }
            a.rgb[(size_t)ray * 3] = w0; a.rgb[(size_t)ray * 3 + 1] = w1; a.rgb[(size_t)ray * 3 + 2] = w2;
            a.disp[ray] = 1.0f / m;
            a.acc[ray] = asum;
            if (a.depth) a.depth[ray] = dsum;
        }
        return;
    }

    // ---- backward: g_i = dL/dw_i, R_i = sum_{j>i} g_j w_j,
    //      dL/dalpha_i = g_i T_i - R_i / t_i
    const float g0 = a.d_rgb[(size_t)ray * 3], g1 = a.d_rgb[(size_t)ray * 3 + 1], g2 = a.d_rgb[(size_t)ray * 3 + 2];
    float gacc = a.d_acc ? a.d_acc[ray] : 0.0f;
    float gdepth = a.d_depth ? a.d_depth[ray] : 0.0f;
    const float* gw = a.d_weights ? a.d_weights + (size_t)ray * S : nullptr;
    if (a.white_bkgd) gacc -= (g0 + g1 + g2);
    if (a.d_disp) {
        const float gd = a.d_disp[ray];
        if (ratio > 1e-10f) {               // disp = acc / depth on this branch
            const float inv = -gd / (m * m);
            gdepth += inv / asum;
            gacc += inv * (-dsum / (asum * asum));
        }
    }
    T = Tstart;
    float segsum = 0.0f;
    for (int i = lo; i < hi; ++i) {
        const float w = s_alpha[i] * T;
        const float c0 = sigmoidf_(raw[4 * i]), c1 = sigmoidf_(raw[4 * i + 1]), c2 = sigmoidf_(raw[4 * i + 2]);
        float g = g0 * c0 + g1 * c1 + g2 * c2 + gacc + gdepth * z[i];
        if (gw) g += gw[i];
        s_gw[i] = g * w;
        segsum += g * w;
        if (a.d_z) a.d_z[(size_t)ray * S + i] = gdepth * w;         // depth integral sum_j w_j z_j: direct term
        // colour gradients are local
        float* dr = a.d_raw + ((size_t)ray * S + i) * 4;
        dr[0] = w * g0 * (c0 * (1.0f - c0));
        dr[1] = w * g1 * (c1 * (1.0f - c1));
        dr[2] = w * g2 * (c2 * (1.0f - c2));
        // stash g*T for the alpha gradient
        s_alpha[i] = g * T;
        T *= s_t[i];
    }
    // suffix sums over later lanes (reverse scan, like ATen's reversed cumsum in cumprod_backward)
    const float suf = wave_incl_scan_add_rev(segsum, lane);
    float R = __shfl_down(suf, 1);          // sum over lanes > this one
    if (lane == 63) R = 0.0f;
    const bool geo = a.d_dirs || a.d_z;
    float ddz = 0.0f, dd_last = 0.0f;
    for (int i = hi - 1; i >= lo; --i) {
        const float dalpha = s_alpha[i] - R / s_t[i];
        a.d_raw[((size_t)ray * S + i) * 4 + 3] = dalpha * s_e[i];
        R += s_gw[i];
        if (geo) {
            // dL/d dist_i = dalpha * relu(sigma) * exp(-relu(sigma) dist)   (dist_i = dz_i |d|, dz_last = 1e10)
            const float dz = (i + 1 < S) ? (z[i + 1] - z[i]) : 1e10f;
            float sg = raw[4 * i + 3];
            if (a.noise) sg = sg + a.noise[(size_t)ray * S + i] * a.noise_std;
            const float rs = fmaxf(sg, 0.0f);
            const float dd = dalpha * (rs * expf(-rs * (dz * dn)));
            ddz += dz * dd;
            s_e[i] = dd;                    // (s_e[i] is not read again)
            if (i == hi - 1) dd_last = dd;
        }
    }
    if (!geo) return;
    const float tot = wave_sum(ddz);
    if (a.d_dirs && lane == 0) {
        const float inv = 1.0f / dn;
        for (int c = 0; c < 3; ++c) a.d_dirs[(size_t)ray * 3 + c] = (dp[c] * inv) * tot;
    }
    if (a.d_z) {
        // dist_i = (z_{i+1} - z_i) |d|: z_i receives |d| (dL/d dist_{i-1} - dL/d dist_i); dist_{lo-1} is the previous lane's last sample
        float prev = __shfl_up(dd_last, 1);
        if (lane == 0) prev = 0.0f;
        for (int i = lo; i < hi; ++i) {
            const float cur = (i + 1 < S) ? s_e[i] : 0.0f;
            a.d_z[(size_t)ray * S + i] += dn * (prev - cur);
            prev = s_e[i];
        }
    }
}

// ------------------------------------------------------------------ distortion loss on the compositing weights
// mip-NeRF 360's regulariser, per ray, with s_i = (z_i - near) / (far - near) (0 when far - near is not > 0), sample i < S-1 owning
// [s_i, s_i+1] (m_i the mid-point, dl_i the length) and the last sample a zero-length interval at s_S-1:
//   L = sum_i sum_j w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 dl_i,      dL/dw_k = 2 sum_j w_j |m_k - m_j| + 2/3 w_k dl_k
// The depths are non-decreasing, so are the m: sum_j w_j |m_k - m_j| = (m_k W_<k - WM_<k) + (WM_>k - m_k W_>k) with exclusive prefixes
// and exclusive suffixes of w and w m -- O(S).  Both are built like composite_ray's scans: sequentially inside the lane's segment,
// across lanes by wave_incl_scan_add / wave_incl_scan_add_rev (the suffix is summed directly, never total minus prefix).
// BWD = false: loss[ray].  BWD = true: d_w[ray][k] (+)= d_loss[ray] dL/dw_k, recomputed from w and z.
// LDS per ray: 2*S floats (fwd) / 4*S floats (bwd); each lane touches only its own segment: no synchronisation
template <bool BWD>
__device__ __forceinline__ void distortion_ray(const DistortionArgs& a, int ray, int lane, float* sm) {
    const int S = a.S;
    const int C = (S + 63) >> 6;
    const int lo = min(lane * C, S), hi = min(lo + C, S);
    const float* w = a.w + (size_t)ray * S;
    const float* z = a.z + (size_t)ray * S;
    const float near = a.near_far[(size_t)ray * a.nf_stride], far = a.near_far[(size_t)ray * a.nf_stride + 1];
    const float span = far - near;
    const bool ok = span > 0.0f;            // (a NaN span fails the comparison too: s = 0, loss 0)
    float* s_w = sm;                // w_i
    float* s_m = sm + S;            // m_i
    float* s_d = sm + 2 * S;        // dl_i                            (bwd)
    float* s_a = sm + 3 * S;        // m_i W_<i - WM_<i                (bwd)

    // pass 1: interval mid-points and lengths, segment sums of w and w m
    float segw = 0.0f, segwm = 0.0f, own = 0.0f;
    float s_cur = (lo < hi && ok) ? (z[lo] - near) / span : 0.0f;
    for (int i = lo; i < hi; ++i) {
        float m = s_cur, dl = 0.0f;
        if (i + 1 < S) {
            const float s_next = ok ? (z[i + 1] - near) / span : 0.0f;
            m = 0.5f * (s_cur + s_next);
            dl = s_next - s_cur;
            s_cur = s_next;
        }
        const float wi = w[i];
        s_w[i] = wi;
        s_m[i] = m;
        if (BWD) s_d[i] = dl; else own += (wi * wi) * dl;
        segw += wi;
        segwm = fmaf(wi, m, segwm);
    }
    const float pw = wave_incl_scan_add(segw, lane), pwm = wave_incl_scan_add(segwm, lane);
    float Wp = __shfl_up(pw, 1), WMp = __shfl_up(pwm, 1);             // sums over the lanes before this one
    if (lane == 0) { Wp = 0.0f; WMp = 0.0f; }
    const float sw = wave_incl_scan_add_rev(segw, lane), swm = wave_incl_scan_add_rev(segwm, lane);
    float Ws = __shfl_down(sw, 1), WMs = __shfl_down(swm, 1);         // sums over the lanes behind this one
    if (lane == 63) { Ws = 0.0f; WMs = 0.0f; }

    // pass 2, ascending: the part of sum_j w_j |m_k - m_j| that lies before k
    float part = 0.0f;
    for (int i = lo; i < hi; ++i) {
        const float wi = s_w[i], m = s_m[i];
        const float before = fmaf(m, Wp, -WMp);         // (one rounding: the two products nearly cancel on a compact ray)
        if (BWD) s_a[i] = before; else part += wi * before;
        Wp += wi;
        WMp = fmaf(wi, m, WMp);
    }
    // pass 3, descending: the part behind k
    const float g = BWD ? a.d_loss[ray] : 0.0f;
    float* dw = BWD ? a.d_w + (size_t)ray * S : nullptr;
    for (int i = hi - 1; i >= lo; --i) {
        const float wi = s_w[i], m = s_m[i];
        const float behind = fmaf(-m, Ws, WMs);
        if (BWD) {
            const float d = g * (2.0f * (s_a[i] + behind) + (2.0f / 3.0f) * (wi * s_d[i]));
            dw[i] = a.accumulate ? dw[i] + d : d;
        } else {
            part += wi * behind;
        }
        Ws += wi;
        WMs = fmaf(wi, m, WMs);
    }
    if (BWD) return;
    part = wave_sum(part);
    own = wave_sum(own);
    if (lane == 0) a.loss[ray] = part + own / 3.0f;
}

// ------------------------------------------------------------------ interlevel loss of proposal weights against a target histogram
// mip-NeRF 360's proposal loss, per ray.  Sample k of either side owns [depth_k, depth_k+1), the last one [depth_last, +inf); target
// interval j and proposal interval i overlap when max(z_j, zp_i) < min(z_j+1, zp_i+1) (a zero-length interval overlaps nothing):
//   bound_j = sum of wp_i over the i overlapping j, ascending i;   L = sum_j max(0, w_j - bound_j)^2 / (w_j + 1e-7)
//   dL/dwp_i = sum over the j overlapping i, ascending j, of -2 max(0, w_j - bound_j) / (w_j + 1e-7)
// Both sides are sorted (the caller's contract), so what overlaps one interval is a contiguous run of the other side -- the intervals that
// end behind its start and begin before its end -- with zero-length intervals inside the run: two binary searches give the run, THE
// PREDICATE ITSELF decides every candidate, and the sum is direct (never a difference of prefix sums).  Sorted partitions overlap in at
// most P + S - 1 pairs: linear work per ray.  The searches return indices in [0, n] whatever the depths hold (NaN, unsorted): every
// candidate index lies inside its row.

// number of entries of v[0..n) that are <= x (UPPER = true) or < x (UPPER = false); v non-decreasing
template <bool UPPER>
__device__ __forceinline__ int interlevel_count(const float* v, int n, float x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const float t = v[mid];
        if (UPPER ? (t <= x) : (t < x)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// sum, in ascending order, of val[k] over the intervals k of the row `edge` [n] that overlap [lo_x, hi_x).  COMP = false: the plain fp32
// sum (bound_j: terms >= 0, so the rounded sum is never below its largest term and an envelope proposal gives exactly 0).  COMP = true:
// the same order with Kahan's carry (the adjoint: a proposal interval gathers up to S terms of size <= 2, and the plain sum's error
// would grow with their count)
template <bool COMP>
__device__ __forceinline__ float interlevel_gather(const float* edge, const float* val, int n, float lo_x, float hi_x) {
    int first = interlevel_count<true>(edge, n, lo_x) - 1;       // the last interval that begins at or before lo_x ends behind it
    if (first < 0) first = 0;
    const int last = interlevel_count<false>(edge, n, hi_x) - 1; // the last interval that begins before hi_x
    float sum = 0.0f, carry = 0.0f;
    for (int k = first; k <= last; ++k) {
        const float e1 = k + 1 < n ? edge[k + 1] : __builtin_inff();
        if (fmaxf(lo_x, edge[k]) < fminf(hi_x, e1)) {
            if (COMP) {
                const float y = val[k] - carry, t = sum + y;
                carry = (t - sum) - y;
                sum = t;
            } else {
                sum += val[k];
            }
        }
    }
    return sum;
}

// BWD = false: loss[ray].  BWD = true: d_wp[ray][i] (+)= d_loss[ray] dL/dwp_i, bound_j recomputed from the inputs.
// LDS per ray: zp | wp (2 P floats), and in the adjoint z | g (2 S floats more, g_j = -2 max(0, w_j - bound_j) / (w_j + 1e-7)).
// Lanes stride over target intervals (forward, and the adjoint's first phase) and over proposal intervals (its second phase).
template <bool BWD, typename Sync>
__device__ __forceinline__ void interlevel_ray(const InterlevelArgs& a, int ray, int lane, float* sm) {
    const int P = a.P, S = a.S;
    const float* wp = a.wp + (size_t)ray * P;
    const float* zp = a.zp + (size_t)ray * P;
    const float* w = a.w + (size_t)ray * S;
    const float* z = a.z + (size_t)ray * S;
    float* s_zp = sm;
    float* s_wp = sm + P;
    float* s_z = sm + 2 * P;            // (bwd)
    float* s_g = sm + 2 * P + S;        // (bwd)
    for (int i = lane; i < P; i += 64) { s_zp[i] = zp[i]; s_wp[i] = wp[i]; }
    Sync::sync();
    float part = 0.0f;
    for (int j = lane; j < S; j += 64) {
        const float z0 = z[j], z1 = j + 1 < S ? z[j + 1] : __builtin_inff();
        const float wj = w[j];
        const float over = fmaxf(0.0f, wj - interlevel_gather<false>(s_zp, s_wp, P, z0, z1));
        if (BWD) { s_z[j] = z0; s_g[j] = -2.0f * over / (wj + 1e-7f); } else part += (over * over) / (wj + 1e-7f);
    }
    if (!BWD) {
        part = wave_sum(part);
        if (lane == 0) a.loss[ray] = part;
        return;
    }
    Sync::sync();
    const float g = a.d_loss[ray];
    float* d_wp = a.d_wp + (size_t)ray * P;
    for (int i = lane; i < P; i += 64) {
        const float d = g * interlevel_gather<true>(s_z, s_g, S, s_zp[i], i + 1 < P ? s_zp[i + 1] : __builtin_inff());
        d_wp[i] = a.accumulate ? d_wp[i] + d : d;
    }
}

// ------------------------------------------------------------------ hierarchical sampling
// LDS: bins[nb] | cdf[nb] | vals[n_in + Nf]
template <typename Sync>
__device__ __forceinline__ void sample_fine_ray(const FineArgs& a, int ray, int lane, float* sm) {
    const int Nf = a.Nf;
    const int nb = a.direct ? a.n_in : a.n_in - 1;      // bins
    const int nw = nb - 1;                              // pdf entries
    const int Sc = a.direct ? 0 : a.n_in;
    const int tot = Sc + Nf;
    float* bins = sm;
    float* cdf = sm + nb;
    float* vals = sm + 2 * nb;
    const float* in0 = a.in0 + (size_t)ray * a.n_in;
    const float* w = a.direct ? a.in1 + (size_t)ray * nw : a.in1 + (size_t)ray * a.n_in + 1;   // weights[1:-1]

    if (a.direct) { for (int i = lane; i < nb; i += 64) bins[i] = in0[i]; }
    else {
        for (int i = lane; i < nb; i += 64) bins[i] = 0.5f * (in0[i + 1] + in0[i]);
        for (int i = lane; i < Sc; i += 64) vals[i] = in0[i];
    }
    float part = 0.0f;
    for (int i = lane; i < nw; i += 64) part += w[i] + 1e-5f;
    const float wsum = wave_sum(part);
    Sync::sync();
    // cdf = [0, cumsum(pdf)]: the ADDITIONS are sequential like torch.cumsum so rounding follows the reference; the divisions
    // (independent) are done by all lanes first
    for (int i = lane; i < nw; i += 64) cdf[i + 1] = (w[i] + 1e-5f) / wsum;
    Sync::sync();
    if (lane == 0) {
        float c = 0.0f;
        cdf[0] = 0.0f;
        for (int i = 0; i < nw; ++i) { c += cdf[i + 1]; cdf[i + 1] = c; }
    }
    Sync::sync();
    float s1 = 0.0f;
    for (int k = lane; k < Nf; k += 64) {
        const float u = a.u ? a.u[(size_t)ray * Nf + k] : (a.u_lin ? a.u_lin[k] : linspace01_at(k, Nf));
        // searchsorted(cdf, u, right=True) = number of entries <= u: the cdf is non-decreasing, so a binary search counts them
        int lo_ = 0, hi_ = nb;
        while (lo_ < hi_) { const int mid = (lo_ + hi_) >> 1; if (cdf[mid] <= u) lo_ = mid + 1; else hi_ = mid; }
        const int idx = lo_;
        const int below = max(idx - 1, 0), above = min(idx, nb - 1);
        const float c0 = cdf[below], c1 = cdf[above];
        float denom = c1 - c0;
        if (denom < 1e-5f) denom = 1.0f;
        const float t = (u - c0) / denom;
        const float smp = bins[below] + t * (bins[above] - bins[below]);
        vals[Sc + k] = smp;
        if (a.z_samples) a.z_samples[(size_t)ray * Nf + k] = smp;
        s1 += smp;
    }
    const float mean = wave_sum(s1) / (float)Nf;
    Sync::sync();
    if (a.z_std) {
        float s2 = 0.0f;
        for (int k = lane; k < Nf; k += 64) { const float d = vals[Sc + k] - mean; s2 += d * d; }
        s2 = wave_sum(s2);
        if (lane == 0) a.z_std[ray] = sqrtf(s2 / (float)Nf);
    }
    if (!a.z_all) return;
    // sorted union (values only are used downstream, run_nerf.py:396: torch.sort(torch.cat([z_vals, z_samples]))).  The
    // coarse depths are ascending already; the fine samples (unsorted when u is random) are sorted in LDS by a bitonic
    // network over the next power of two (padding = +inf), then every element finds its place in the union by one binary
    // search in the OTHER list (coarse before fine on ties: a stable merge).  O(n log^2 n) instead of the O(n^2) rank count;
    // the output is the same sorted sequence.
    float* fs = vals + Sc;
    int np2 = 1;
    while (np2 < Nf) np2 <<= 1;
    for (int k = Nf + lane; k < np2; k += 64) fs[k] = __int_as_float(0x7f800000);
    Sync::sync();
    for (int size = 2; size <= np2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = lane; t < (np2 >> 1); t += 64) {
                const int i = ((t / stride) * (stride << 1)) + (t % stride), j = i + stride;
                const bool up = ((i & size) == 0);
                const float x = fs[i], y = fs[j];
                if ((x > y) == up) { fs[i] = y; fs[j] = x; }
            }
            Sync::sync();
        }
    float* zo = a.z_all + (size_t)ray * tot;
    for (int i = lane; i < Sc; i += 64) {             // coarse element i: + number of fine samples strictly below it
        const float x = vals[i];
        int lo_ = 0, hi_ = Nf;
        while (lo_ < hi_) { const int mid = (lo_ + hi_) >> 1; if (fs[mid] < x) lo_ = mid + 1; else hi_ = mid; }
        zo[i + lo_] = x;
    }
    for (int k = lane; k < Nf; k += 64) {             // fine element k (sorted position): + number of coarse depths <= it
        const float x = fs[k];
        int lo_ = 0, hi_ = Sc;
        while (lo_ < hi_) { const int mid = (lo_ + hi_) >> 1; if (vals[mid] <= x) lo_ = mid + 1; else hi_ = mid; }
        zo[k + lo_] = x;
    }
}

}  // namespace nerf
