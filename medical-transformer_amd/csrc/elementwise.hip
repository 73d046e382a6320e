// elementwise.hip -- the streaming kernels between the convolutions and the attention layers:
//   BatchNorm2d apply (+residual, +ReLU) and its backward   (axialnet.py:285-300, 475-483)
//   bilinear x2 upsample + ReLU + skip-add                   (axialnet.py:493-501, 650-652, 690-698)
//   LoGo patch gather / merge                                (axialnet.py:658-702)
//   cross-entropy loss                                       (metrics.py:17-20)
//   Adam with coupled L2 weight decay over a flat buffer     (train.py:111-112,161)
//   sliding-window gather / blend for images larger than the network input (not in the reference)
//   test-time augmentation: the flipped / transposed views of a batch and the mean of their logits (not in the reference)
//   joint augmentation of uint8 batches: crop, flip, colour jitter, affine (utils.py:70-98)
//   exact squared Euclidean distance transform of uint8 masks, for the surface-distance scores (not in the reference)
// All HBM-bound: one element per lane, NCHW rows coalesced, per-channel constants via scalar loads.
#include "medt_kernels.h"
#include <stdint.h>
#include <stdlib.h>

namespace medt {

static inline unsigned grid1d(size_t total) { return (unsigned)((total + MEDT_THREADS - 1) / MEDT_THREADS); }

// y = [relu]( z*scale[g,c] + shift[g,c] [+ res] )         one lane per element of (N,C,HW)
__global__ __launch_bounds__(MEDT_THREADS) void bn_apply_act_kernel(const float* __restrict__ z, BnStats st,
                                                                    const float* __restrict__ res,
                                                                    float* __restrict__ y, int C, int HW, int npg,
                                                                    int relu, size_t total) {
    const size_t idx = (size_t)blockIdx.x * MEDT_THREADS + threadIdx.x;
    if (idx >= total) return;
    const size_t nc = idx / HW;
    const int c = (int)(nc % C), n = (int)(nc / C);
    const int gc = (n / npg) * C + c;
    float v = fmaf(z[idx], st.scale[gc], st.shift[gc]);
    if (res) v += res[idx];
    if (relu) v = fmaxf(v, 0.f);
    y[idx] = v;
}

int bn_apply_act(const float* z, BnStats st, const float* res, float* y, int N, int C, int HW, int groups, int relu,
                 hipStream_t s) {
    const size_t total = (size_t)N * C * HW;
    hipLaunchKernelGGL(bn_apply_act_kernel, dim3(grid1d(total)), dim3(MEDT_THREADS), 0, s, z, st, res, y, C, HW,
                       N / groups, relu, total);
    return launch_status("bn_apply_act");
}

// bn_finalize + bn_apply_act in one launch: every workgroup re-derives the statistics of ITS (group, channel) from the
// convolution's partial sums (ppg pairs of doubles: one round trip) and then normalises its slice of that population;
// part 0 saves mean / rstd / scale / shift for backward.  What is left of the finalisation -- the running-statistics
// recurrence over the groups -- is off the layer chain (recorded, or issued right behind when no queue is bound).
struct BnFinApplyArgs {
    const float *z, *partials, *weight, *bias, *running_mean, *running_var, *res;
    float* y;
    BnStats st;
    int C, HW, npg, ppg, parts, relu, training, vec4;     // vec4: HW % 4 == 0 and z / res / y 16-byte aligned
    double count;
    float eps;
};
constexpr int BFA_PER_THREAD = 16;
// (the body takes its block coordinates as arguments: bn_fin_apply_pair_kernel below runs two problems in one grid)
__device__ __forceinline__ void bn_fin_apply_body(const BnFinApplyArgs& a, double* redd, int bx, int by) {
    const int grp = bx / a.parts, part = bx - grp * a.parts, c = by, tid = threadIdx.x;
    const int gc = grp * a.C + c;
    const float gam = a.weight[c], bet = a.bias[c];
    float mean_f, rstd_f, scale, shift;
    if (a.training) {
        const double* pd = reinterpret_cast<const double*>(a.partials);
        double s = 0.0, ss = 0.0;
        for (int p = tid; p < a.ppg; p += MEDT_THREADS) {
            const double* q = pd + ((size_t)(grp * a.ppg + p) * a.C + c) * 2;
            s += q[0];
            ss += q[1];
        }
        s = wave_sum_d(s);
        ss = wave_sum_d(ss);
        if ((tid & 63) == 0) { redd[(tid >> 6) * 2] = s; redd[(tid >> 6) * 2 + 1] = ss; }
        __syncthreads();
        s = 0.0;
        ss = 0.0;
#pragma unroll
        for (int w = 0; w < MEDT_WAVES; ++w) { s += redd[w * 2]; ss += redd[w * 2 + 1]; }
        const double mean = s / a.count;
        double var = ss / a.count - mean * mean;
        if (var < 0.0) var = 0.0;
        const double rstd = 1.0 / sqrt(var + (double)a.eps);
        mean_f = (float)mean;
        rstd_f = (float)rstd;
        scale = (float)(gam * rstd);
        shift = (float)(bet - mean * gam * rstd);
    } else {
        mean_f = a.running_mean[c];
        rstd_f = (float)(1.0 / sqrt((double)a.running_var[c] + (double)a.eps));
        scale = gam * rstd_f;
        shift = bet - mean_f * gam * rstd_f;
    }
    if (part == 0 && tid == 0) {
        a.st.mean[gc] = mean_f;
        a.st.rstd[gc] = rstd_f;
        a.st.scale[gc] = scale;
        a.st.shift[gc] = shift;
    }
    const int HW = a.HW, P = a.npg * HW;
    const int q0 = part * (MEDT_THREADS * BFA_PER_THREAD);
    const int q1 = q0 + MEDT_THREADS * BFA_PER_THREAD < P ? q0 + MEDT_THREADS * BFA_PER_THREAD : P;
    if (a.vec4) {
        for (int q = q0 + 4 * tid; q < q1; q += 4 * MEDT_THREADS) {
            const int ni = q / HW, p = q - ni * HW;
            const size_t idx = ((size_t)(grp * a.npg + ni) * a.C + c) * HW + p;
            const float4 zz = *reinterpret_cast<const float4*>(a.z + idx);
            float4 v;
            v.x = fmaf(zz.x, scale, shift);
            v.y = fmaf(zz.y, scale, shift);
            v.z = fmaf(zz.z, scale, shift);
            v.w = fmaf(zz.w, scale, shift);
            if (a.res) {
                const float4 r = *reinterpret_cast<const float4*>(a.res + idx);
                v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
            }
            if (a.relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
            *reinterpret_cast<float4*>(a.y + idx) = v;
        }
    } else {
        for (int q = q0 + tid; q < q1; q += MEDT_THREADS) {
            const int ni = q / HW, p = q - ni * HW;
            const size_t idx = ((size_t)(grp * a.npg + ni) * a.C + c) * HW + p;
            float v = fmaf(a.z[idx], scale, shift);
            if (a.res) v += a.res[idx];
            if (a.relu) v = fmaxf(v, 0.f);
            a.y[idx] = v;
        }
    }
}

__global__ __launch_bounds__(MEDT_THREADS) void bn_fin_apply_kernel(BnFinApplyArgs a) {
    MEDT_STATIC_SHARED double redd[2 * MEDT_WAVES];
    bn_fin_apply_body(a, redd, blockIdx.x, blockIdx.y);
}

// Two bn_fin_apply problems in one launch, as a two-entry job table: blocks [0, blocksA) are problem 0's grid, row-major
// (groups * parts, C), the rest problem 1's -- each keeps its own grid shape inside its range; the choice is uniform over the workgroup
struct BnFinApplyPair { BnFinApplyArgs job[2]; int gx[2]; int blocksA; };
__global__ __launch_bounds__(MEDT_THREADS) void bn_fin_apply_pair_kernel(BnFinApplyPair p) {
    MEDT_STATIC_SHARED double redd[2 * MEDT_WAVES];
    const int second = (int)blockIdx.x >= p.blocksA ? 1 : 0;
    const int local = (int)blockIdx.x - (second ? p.blocksA : 0), gx = p.gx[second];
    const int by = local / gx;
    bn_fin_apply_body(p.job[second], redd, local - by * gx, by);
}

static BnFinApplyArgs bn_fin_apply_args(const float* z, const float* partials, int ppg, double count, const medt_bn_ptrs& bn, float eps,
                                        int training, BnStats st, const float* res, float* y, int N, int C, int HW, int groups,
                                        int relu) {
    BnFinApplyArgs a;
    a.z = z; a.partials = partials; a.weight = bn.weight; a.bias = bn.bias; a.running_mean = bn.running_mean;
    a.running_var = bn.running_var; a.res = res; a.y = y; a.st = st; a.C = C; a.HW = HW; a.npg = N / groups; a.ppg = ppg;
    a.parts = cdiv(a.npg * HW, MEDT_THREADS * BFA_PER_THREAD); a.relu = relu; a.training = training; a.count = count;
    a.vec4 = ((HW & 3) == 0 && (((uintptr_t)z | (uintptr_t)y | (uintptr_t)res) & 15) == 0) ? 1 : 0;
    a.eps = eps;
    return a;
}

int bn_fin_apply(const float* z, const float* partials, int ppg, double count, const medt_bn_ptrs& bn, float eps, int training,
                 BnStats st, const float* res, float* y, int N, int C, int HW, int groups, int relu, hipStream_t s) {
    const BnFinApplyArgs a = bn_fin_apply_args(z, partials, ppg, count, bn, eps, training, st, res, y, N, C, HW, groups, relu);
    hipLaunchKernelGGL(bn_fin_apply_kernel, dim3(groups * a.parts, C), dim3(MEDT_THREADS), 0, s, a);
    return launch_status("bn_fin_apply");
}

int bn_fin_apply_pair(const BnFinApplyProblem& a, const BnFinApplyProblem& b, hipStream_t s) {
    const BnFinApplyProblem* in[2] = {&a, &b};
    BnFinApplyPair p;
    for (int i = 0; i < 2; ++i) {
        const BnFinApplyProblem& q = *in[i];
        p.job[i] = bn_fin_apply_args(q.z, q.partials, q.ppg, q.count, *q.bn, q.eps, q.training, q.st, q.res, q.y, q.N, q.C, q.HW,
                                     q.groups, q.relu);
        p.gx[i] = q.groups * p.job[i].parts;
    }
    p.blocksA = p.gx[0] * a.C;
    hipLaunchKernelGGL(bn_fin_apply_pair_kernel, dim3((unsigned)(p.blocksA + p.gx[1] * b.C)), dim3(MEDT_THREADS), 0, s, p);
    return launch_status("bn_fin_apply_pair");
}

// g = dy * (y > 0 if relu) ; partials[group][part][C][2] = [sum g, sum g*zhat]     grid (groups*ppg, C),
// lanes over the flattened (image, pixel) positions of one group and one channel
__global__ __launch_bounds__(MEDT_THREADS) void bn_act_bwd_stats_kernel(const float* __restrict__ dy,
                                                                        const float* __restrict__ y,
                                                                        const float* __restrict__ z, BnStats st,
                                                                        float* __restrict__ g,
                                                                        float* __restrict__ partials, int C, int HW,
                                                                        int npg, int relu) {
    MEDT_STATIC_SHARED float red[MEDT_WAVES * 2];
    const int per_group = npg * HW, ppg = (per_group + MEDT_THREADS - 1) / MEDT_THREADS;
    const int grp = blockIdx.x / ppg, part = blockIdx.x - grp * ppg, c = blockIdx.y;
    const int q = part * MEDT_THREADS + threadIdx.x;
    float v[2] = {0.f, 0.f};
    if (q < per_group) {
        const int ni = q / HW, p = q - ni * HW;
        const int gc = grp * C + c;
        const size_t idx = ((size_t)(grp * npg + ni) * C + c) * HW + p;
        float d = dy[idx];
        if (relu && !(y[idx] > 0.f)) d = 0.f;
        if (g) g[idx] = d;
        v[0] = d;
        v[1] = d * ((z[idx] - st.mean[gc]) * st.rstd[gc]);
    }
    block_sum<2>(v, red, partials + ((size_t)blockIdx.x * C + c) * 2);
}

int bn_act_bwd_stats(const float* dy, const float* y, const float* z, BnStats st, float* g, float* partials, int N, int C,
                     int HW, int groups, int relu, hipStream_t s) {
    const int ppg = cdiv((N / groups) * HW, MEDT_THREADS);
    hipLaunchKernelGGL(bn_act_bwd_stats_kernel, dim3(groups * ppg, C), dim3(MEDT_THREADS), 0, s, dy, y, z, st, g,
                       partials, C, HW, N / groups, relu);
    return launch_status("bn_act_bwd_stats");
}

// dz = c0*g + c1*z + c2   (coef [group][C][3])
__global__ __launch_bounds__(MEDT_THREADS) void bn_bwd_apply_kernel(const float* __restrict__ g,
                                                                    const float* __restrict__ z,
                                                                    const float* __restrict__ coef,
                                                                    float* __restrict__ dz, int C, int HW, int npg,
                                                                    size_t total) {
    const size_t idx = (size_t)blockIdx.x * MEDT_THREADS + threadIdx.x;
    if (idx >= total) return;
    const size_t nc = idx / HW;
    const int c = (int)(nc % C), n = (int)(nc / C);
    const float* cf = coef + ((size_t)(n / npg) * C + c) * 3;
    dz[idx] = fmaf(cf[0], g[idx], fmaf(cf[1], z[idx], cf[2]));
}

int bn_bwd_apply(const float* g, const float* z, const float* coef, float* dz, int N, int C, int HW, int groups,
                 hipStream_t s) {
    const size_t total = (size_t)N * C * HW;
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(grid1d(total)), dim3(MEDT_THREADS), 0, s, g, z, coef, dz, C, HW,
                       N / groups, total);
    return launch_status("bn_bwd_apply");
}

// out = a * (y > 0)            (ReLU backward by output sign)
__global__ __launch_bounds__(MEDT_THREADS) void relu_mask_kernel(const float* __restrict__ a, const float* __restrict__ y,
                                                                 float* __restrict__ out, size_t total) {
    const size_t i = (size_t)blockIdx.x * MEDT_THREADS + threadIdx.x;
    if (i < total) out[i] = y[i] > 0.f ? a[i] : 0.f;
}

int relu_mask(const float* a, const float* y, float* out, size_t total, hipStream_t s) {
    hipLaunchKernelGGL(relu_mask_kernel, dim3(grid1d(total)), dim3(MEDT_THREADS), 0, s, a, y, out, total);
    return launch_status("relu_mask");
}

// y = relu(x)  /  y = relu(x) in place of a previous ReLU-free tensor
__global__ __launch_bounds__(MEDT_THREADS) void relu_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                            size_t total) {
    const size_t i = (size_t)blockIdx.x * MEDT_THREADS + threadIdx.x;
    if (i < total) y[i] = fmaxf(x[i], 0.f);
}

int relu_fwd(const float* x, float* y, size_t total, hipStream_t s) {
    hipLaunchKernelGGL(relu_kernel, dim3(grid1d(total)), dim3(MEDT_THREADS), 0, s, x, y, total);
    return launch_status("relu");
}

// --------------------------------------------------------------------------- //
// bilinear x2 (align_corners=False) + ReLU + skip-add
// --------------------------------------------------------------------------- //
struct Lerp { int i0, i1; float l; };
__device__ __forceinline__ Lerp src_index(int o, int n_in) {
    float s = 0.5f * ((float)o + 0.5f) - 0.5f;         // aten area_pixel_compute_source_index, scale = 1/2
    if (s < 0.f) s = 0.f;
    Lerp r;
    r.i0 = (int)s;
    r.i1 = r.i0 + (r.i0 < n_in - 1 ? 1 : 0);
    r.l = s - (float)r.i0;
    return r;
}

// one interpolated value from its four sources: explicit FMAs, so that the forward value and the backward's ReLU mask
// (recomputed from registers) are the same arithmetic whatever the compiler contracts
__device__ __forceinline__ float up_value(float v00, float v01, float v10, float v11, float lh, float lw) {
    const float h0 = 1.f - lh, w0 = 1.f - lw;
    const float t0 = fmaf(lw, v01, w0 * v00), t1 = fmaf(lw, v11, w0 * v10);
    return fmaf(lh, t1, h0 * t0);
}

__device__ __forceinline__ float up_sample(const float* __restrict__ xp, int H, int W, int ho, int wo) {
    const Lerp a = src_index(ho, H), b = src_index(wo, W);
    return up_value(xp[a.i0 * W + b.i0], xp[a.i0 * W + b.i1], xp[a.i1 * W + b.i0], xp[a.i1 * W + b.i1], a.l, b.l);
}

__global__ __launch_bounds__(MEDT_THREADS) void up2x_relu_add_kernel(const float* __restrict__ x,
                                                                     const float* __restrict__ skip,
                                                                     float* __restrict__ y, int H, int W, size_t total) {
    const size_t idx = (size_t)blockIdx.x * MEDT_THREADS + threadIdx.x;
    if (idx >= total) return;
    const int Wo = 2 * W, Ho = 2 * H;
    const int wo = (int)(idx % Wo), ho = (int)((idx / Wo) % Ho);
    const size_t nc = idx / ((size_t)Wo * Ho);
    float v = fmaxf(up_sample(x + nc * H * W, H, W, ho, wo), 0.f);
    if (skip) v += skip[idx];
    y[idx] = v;
}

// Four consecutive output columns per lane (W even): they interpolate between input columns 2t-1 .. 2t+2 of two rows, so
// eight loads serve four outputs and skip / y move as float4.  Same Lerp values and the same up_value arithmetic as the
// scalar kernel (the border clamps coincide with src_index's).
__global__ __launch_bounds__(MEDT_THREADS) void up2x_relu_add4_kernel(const float* __restrict__ x,
                                                                      const float* __restrict__ skip,
                                                                      float* __restrict__ y, int H, int W, size_t total4) {
    const size_t idx = (size_t)blockIdx.x * MEDT_THREADS + threadIdx.x;
    if (idx >= total4) return;
    const int Wq = W / 2, Ho = 2 * H;
    const int t = (int)(idx % Wq), ho = (int)((idx / Wq) % Ho);
    const size_t nc = idx / ((size_t)Wq * Ho);
    const float* xp = x + nc * H * W;
    const Lerp a = src_index(ho, H);
    const int cc[4] = {max(2 * t - 1, 0), 2 * t, 2 * t + 1, min(2 * t + 2, W - 1)};
    float r0[4], r1[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        r0[k] = xp[a.i0 * W + cc[k]];
        r1[k] = xp[a.i1 * W + cc[k]];
    }
    constexpr int C0[4] = {0, 1, 1, 2};
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const Lerp b = src_index(4 * t + k, W);
        v[k] = fmaxf(up_value(r0[C0[k]], r0[C0[k] + 1], r1[C0[k]], r1[C0[k] + 1], a.l, b.l), 0.f);
    }
    const size_t o = (nc * Ho + ho) * (size_t)(2 * W) + 4 * t;
    if (skip) {
        const float4 sk = *reinterpret_cast<const float4*>(skip + o);
        v[0] += sk.x; v[1] += sk.y; v[2] += sk.z; v[3] += sk.w;
    }
    *reinterpret_cast<float4*>(y + o) = make_float4(v[0], v[1], v[2], v[3]);
}

int up2x_relu_add_fwd(const float* x, const float* skip, float* y, int NC, int H, int W, hipStream_t s) {
    const size_t total = (size_t)NC * 4 * H * W;
    static const bool vec = true;
    if (vec && (W & 1) == 0 && ((uintptr_t)y & 15) == 0 && (!skip || ((uintptr_t)skip & 15) == 0)) {
        hipLaunchKernelGGL(up2x_relu_add4_kernel, dim3(grid1d(total / 4)), dim3(MEDT_THREADS), 0, s, x, skip, y, H, W, total / 4);
        return launch_status("up2x_relu_add4");
    }
    hipLaunchKernelGGL(up2x_relu_add_kernel, dim3(grid1d(total)), dim3(MEDT_THREADS), 0, s, x, skip, y, H, W, total);
    return launch_status("up2x_relu_add");
}

// dx[h,w] = sum over the (<=16) output pixels whose interpolation touches (h,w) of weight * dy * [up(x) > 0].
// The 16 output pixels (rows 2h-1 .. 2h+2, columns 2w-1 .. 2w+2) interpolate between the 3 x 3 neighbourhood of (h,w):
// rows (h-1,h) for the first two, (h,h+1) for the last two (the border clamps coincide with src_index's), so the
// neighbourhood is loaded once and the 16 mask values come from registers (80 -> 25 loads per lane).
__global__ __launch_bounds__(MEDT_THREADS) void up2x_relu_bwd_kernel(const float* __restrict__ x,
                                                                     const float* __restrict__ dy,
                                                                     float* __restrict__ dx, int H, int W, size_t total) {
    const size_t idx = (size_t)blockIdx.x * MEDT_THREADS + threadIdx.x;
    if (idx >= total) return;
    const int w = (int)(idx % W), h = (int)((idx / W) % H);
    const size_t nc = idx / ((size_t)W * H);
    const float* xp = x + nc * H * W;
    const float* dp = dy + nc * 4 * H * W;
    const int Ho = 2 * H, Wo = 2 * W;
    const int rr[3] = {max(h - 1, 0), h, min(h + 1, H - 1)}, cc[3] = {max(w - 1, 0), w, min(w + 1, W - 1)};
    float xs[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) xs[a][b] = xp[rr[a] * W + cc[b]];
    float lw[4], ww[4];
    bool wok[4];
#pragma unroll
    for (int kw = 0; kw < 4; ++kw) {
        const int wo = 2 * w - 1 + kw;
        const Lerp b = src_index(wo < 0 ? 0 : wo, W);
        lw[kw] = b.l;
        ww[kw] = (b.i0 == w ? 1.f - b.l : 0.f) + (b.i1 == w ? b.l : 0.f);
        wok[kw] = wo >= 0 && wo < Wo && ww[kw] != 0.f;
    }
    float acc = 0.f;
#pragma unroll
    for (int kh = 0; kh < 4; ++kh) {
        const int ho = 2 * h - 1 + kh;
        if (ho < 0 || ho >= Ho) continue;
        const Lerp a = src_index(ho, H);
        const float wh = (a.i0 == h ? 1.f - a.l : 0.f) + (a.i1 == h ? a.l : 0.f);
        if (wh == 0.f) continue;
        constexpr int R0[4] = {0, 0, 1, 1};
        const int r0 = R0[kh];
#pragma unroll
        for (int kw = 0; kw < 4; ++kw) {
            if (!wok[kw]) continue;
            const int c0 = R0[kw];
            const float up = up_value(xs[r0][c0], xs[r0][c0 + 1], xs[r0 + 1][c0], xs[r0 + 1][c0 + 1], a.l, lw[kw]);
            if (up > 0.f) acc = fmaf(wh * ww[kw], dp[(size_t)ho * Wo + 2 * w - 1 + kw], acc);
        }
    }
    dx[idx] = acc;
}

int up2x_relu_bwd(const float* x, const float* dy, float* dx, int NC, int H, int W, hipStream_t s) {
    const size_t total = (size_t)NC * H * W;
    hipLaunchKernelGGL(up2x_relu_bwd_kernel, dim3(grid1d(total)), dim3(MEDT_THREADS), 0, s, x, dy, dx, H, W, total);
    return launch_status("up2x_relu_bwd");
}

// --------------------------------------------------------------------------- //
// LoGo patches: gather (N,C,S,S) -> (G*G*N, C, P, P) patch-major; merge y = x + x_loc
// --------------------------------------------------------------------------- //
__global__ __launch_bounds__(MEDT_THREADS) void patch_gather_kernel(const float* __restrict__ x, float* __restrict__ xp,
                                                                    int N, int C, int S, int P, int G, size_t total) {
    const size_t idx = (size_t)blockIdx.x * MEDT_THREADS + threadIdx.x;
    if (idx >= total) return;
    const int w = (int)(idx % P), h = (int)((idx / P) % P);
    const int c = (int)((idx / ((size_t)P * P)) % C);
    const int b = (int)(idx / ((size_t)P * P * C));         // b = patch*N + n
    const int patch = b / N, n = b - patch * N;
    const int pi = patch / G, pj = patch - pi * G;
    xp[idx] = x[(((size_t)n * C + c) * S + pi * P + h) * S + pj * P + w];
}

int patch_gather(const float* x, float* xp, int N, int C, int S, int P, int G, hipStream_t s) {
    const size_t total = (size_t)G * G * N * C * P * P;
    hipLaunchKernelGGL(patch_gather_kernel, dim3(grid1d(total)), dim3(MEDT_THREADS), 0, s, x, xp, N, C, S, P, G, total);
    return launch_status("patch_gather");
}

// y = x + x_loc, x_loc = x with the G x G grid of P-px patches (top-left G*P square) overwritten by yp   (:658,:700-702)
__global__ __launch_bounds__(MEDT_THREADS) void logo_merge_kernel(const float* __restrict__ x,
                                                                  const float* __restrict__ yp, float* __restrict__ y,
                                                                  int N, int C, int S, int P, int G, size_t total) {
    const size_t idx = (size_t)blockIdx.x * MEDT_THREADS + threadIdx.x;
    if (idx >= total) return;
    const int w = (int)(idx % S), h = (int)((idx / S) % S);
    const int c = (int)((idx / ((size_t)S * S)) % C);
    const int n = (int)(idx / ((size_t)S * S * C));
    const float xv = x[idx];
    float loc = xv;
    if (h < G * P && w < G * P) {
        const int patch = (h / P) * G + (w / P);
        loc = yp[((((size_t)patch * N + n) * C + c) * P + (h % P)) * P + (w % P)];
    }
    y[idx] = xv + loc;
}

int logo_merge_fwd(const float* x, const float* yp, float* y, int N, int C, int S, int P, int G, hipStream_t s) {
    const size_t total = (size_t)N * C * S * S;
    hipLaunchKernelGGL(logo_merge_kernel, dim3(grid1d(total)), dim3(MEDT_THREADS), 0, s, x, yp, y, N, C, S, P, G, total);
    return launch_status("logo_merge");
}

// dx = dy * (inside patches ? 1 : 2);  dyp = gather(dy)
__global__ __launch_bounds__(MEDT_THREADS) void logo_merge_bwd_kernel(const float* __restrict__ dy,
                                                                      float* __restrict__ dx, float* __restrict__ dyp,
                                                                      int N, int C, int S, int P, int G, size_t total) {
    const size_t idx = (size_t)blockIdx.x * MEDT_THREADS + threadIdx.x;
    if (idx >= total) return;
    const int w = (int)(idx % S), h = (int)((idx / S) % S);
    const int c = (int)((idx / ((size_t)S * S)) % C);
    const int n = (int)(idx / ((size_t)S * S * C));
    const float d = dy[idx];
    if (h < G * P && w < G * P) {
        const int patch = (h / P) * G + (w / P);
        dyp[((((size_t)patch * N + n) * C + c) * P + (h % P)) * P + (w % P)] = d;
        dx[idx] = d;
    } else {
        dx[idx] = 2.f * d;
    }
}

int logo_merge_bwd(const float* dy, float* dx, float* dyp, int N, int C, int S, int P, int G, hipStream_t s) {
    const size_t total = (size_t)N * C * S * S;
    hipLaunchKernelGGL(logo_merge_bwd_kernel, dim3(grid1d(total)), dim3(MEDT_THREADS), 0, s, dy, dx, dyp, N, C, S, P, G,
                       total);
    return launch_status("logo_merge_bwd");
}

// --------------------------------------------------------------------------- //
// cross entropy (mean over non-ignored pixels), K classes on dim 1
// --------------------------------------------------------------------------- //
__global__ __launch_bounds__(MEDT_THREADS) void ce_fwd_kernel(const float* __restrict__ logits,
                                                              const int64_t* __restrict__ target,
                                                              float* __restrict__ partials, int K, int HW, int ignore,
                                                              size_t total) {
    MEDT_STATIC_SHARED float red[MEDT_WAVES * 3];
    const size_t idx = (size_t)blockIdx.x * MEDT_THREADS + threadIdx.x;     // over N*HW
    float v[3] = {0.f, 0.f, 0.f};
    if (idx < total) {
        const size_t n = idx / HW, p = idx - n * HW;
        const int64_t t = target[idx];
        if (t != ignore && (t < 0 || t >= K)) v[2] = 1.f;      // F.cross_entropy raises on these: counted, reported
        if (t != ignore && t >= 0 && t < K) {
            const float* lp = logits + n * K * HW + p;
            float m = lp[0];
            for (int k = 1; k < K; ++k) m = fmaxf(m, lp[(size_t)k * HW]);
            float sum = 0.f;
            for (int k = 0; k < K; ++k) sum += __expf(lp[(size_t)k * HW] - m);
            v[0] = m + __logf(sum) - lp[(size_t)t * HW];
            v[1] = 1.f;
        }
    }
    block_sum<3>(v, red, partials + (size_t)blockIdx.x * 3);
}

// loss_out[0] = sum/count, loss_out[1] = count, loss_out[2] = number of out-of-range targets
__global__ __launch_bounds__(64) void ce_finalize_kernel(const float* __restrict__ partials, int nparts,
                                                         float* __restrict__ loss_out) {
    double s = 0.0, c = 0.0, b = 0.0;
    for (int p = threadIdx.x; p < nparts; p += 64) {
        s += (double)partials[3 * p];
        c += (double)partials[3 * p + 1];
        b += (double)partials[3 * p + 2];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o, 64); c += __shfl_xor(c, o, 64); b += __shfl_xor(b, o, 64); }
    if (threadIdx.x == 0) {
        loss_out[0] = (float)(s / c);
        loss_out[1] = (float)c;
        loss_out[2] = (float)b;
    }
}

int ce_parts(size_t npix) { return (int)grid1d(npix); }

int ce_fwd(const float* logits, const int64_t* target, float* partials, float* loss_out, int N, int K, int HW, int ignore,
           hipStream_t s) {
    const size_t total = (size_t)N * HW;
    hipLaunchKernelGGL(ce_fwd_kernel, dim3(grid1d(total)), dim3(MEDT_THREADS), 0, s, logits, target, partials, K, HW,
                       ignore, total);
    int rc = launch_status("ce_fwd");
    if (rc) return rc;
    hipLaunchKernelGGL(ce_finalize_kernel, dim3(1), dim3(64), 0, s, partials, (int)grid1d(total), loss_out);
    return launch_status("ce_finalize");
}

// dlogits[n,k,p] = (softmax_k - [k == t]) * dloss / count
__global__ __launch_bounds__(MEDT_THREADS) void ce_bwd_kernel(const float* __restrict__ logits,
                                                              const int64_t* __restrict__ target,
                                                              const float* __restrict__ loss_out,
                                                              const float* __restrict__ dloss,
                                                              float* __restrict__ dlogits, int K, int HW, int ignore,
                                                              size_t total) {
    const size_t idx = (size_t)blockIdx.x * MEDT_THREADS + threadIdx.x;
    if (idx >= total) return;
    const size_t n = idx / HW, p = idx - n * HW;
    const int64_t t = target[idx];
    const float* lp = logits + n * K * HW + p;
    float* dp = dlogits + n * K * HW + p;
    if (t == ignore || t < 0 || t >= K) {
        for (int k = 0; k < K; ++k) dp[(size_t)k * HW] = 0.f;
        return;
    }
    const float scale = (dloss ? dloss[0] : 1.f) / loss_out[1];
    float m = lp[0];
    for (int k = 1; k < K; ++k) m = fmaxf(m, lp[(size_t)k * HW]);
    float sum = 0.f;
    for (int k = 0; k < K; ++k) sum += __expf(lp[(size_t)k * HW] - m);
    const float inv = 1.f / sum;
    for (int k = 0; k < K; ++k) {
        const float pk = __expf(lp[(size_t)k * HW] - m) * inv;
        dp[(size_t)k * HW] = (pk - (k == t ? 1.f : 0.f)) * scale;
    }
}

int ce_bwd(const float* logits, const int64_t* target, const float* loss_out, const float* dloss, float* dlogits, int N,
           int K, int HW, int ignore, hipStream_t s) {
    const size_t total = (size_t)N * HW;
    hipLaunchKernelGGL(ce_bwd_kernel, dim3(grid1d(total)), dim3(MEDT_THREADS), 0, s, logits, target, loss_out, dloss,
                       dlogits, K, HW, ignore, total);
    return launch_status("ce_bwd");
}

// --------------------------------------------------------------------------- //
// segmentation loss = ce_scale * class-weighted cross entropy + dice_scale * soft Dice (per image, per class)
//   three launches like the plain cross entropy above: partial sums per workgroup, one finalize, one pointwise backward.
//   KD = 0: cross entropy only, any K (run-time class loop).  KD = K in [2, 8]: Dice on, the per-class sums live in registers.
//   The grid runs over (image, block of 256 pixels of that image): a workgroup never straddles two images, so the Dice
//   sums of an image are the sums of its own bpi = ceil(HW / 256) partial rows and the backward's per-image coefficients are
//   workgroup-uniform.  No float atomics anywhere: every sum has a fixed order (block_sum, then double in the finalize).
// --------------------------------------------------------------------------- //
// partials [N][bpi][3 + 3 KD] = {sum w nll, sum w, targets outside [0,K) that are not `ignore`, I_k.., P_k.., T_k..}
template <int KD>
__global__ __launch_bounds__(MEDT_THREADS) void seg_loss_fwd_kernel(const float* __restrict__ logits,
                                                                    const int64_t* __restrict__ target,
                                                                    const float* __restrict__ weight,
                                                                    float* __restrict__ partials, int K, int HW, int bpi,
                                                                    int ignore) {
    constexpr int NV = 3 + 3 * KD;
    MEDT_STATIC_SHARED float red[MEDT_WAVES * NV];
    const int n = blockIdx.x / bpi;
    const int p = (blockIdx.x - n * bpi) * MEDT_THREADS + threadIdx.x;       // pixel within image n
    float v[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = 0.f;
    if (p < HW) {
        const int64_t t = target[(size_t)n * HW + p];
        const bool valid = t != ignore && t >= 0 && t < K;
        if (t != ignore && !valid) v[2] = 1.f;                 // F.cross_entropy raises on these: counted, reported
        if (valid) {
            const float* lp = logits + (size_t)n * K * HW + p;
            const float w = weight ? weight[t] : 1.f;
            if constexpr (KD == 0) {
                float m = lp[0];
                for (int k = 1; k < K; ++k) m = fmaxf(m, lp[(size_t)k * HW]);
                float sum = 0.f;
                for (int k = 0; k < K; ++k) sum += __expf(lp[(size_t)k * HW] - m);
                v[0] = w * (m + __logf(sum) - lp[(size_t)t * HW]);
            } else {
                float l[KD];
#pragma unroll
                for (int k = 0; k < KD; ++k) l[k] = lp[(size_t)k * HW];
                float m = l[0], lt = l[0];
#pragma unroll
                for (int k = 1; k < KD; ++k) { m = fmaxf(m, l[k]); lt = (k == t) ? l[k] : lt; }
                float sum = 0.f;
#pragma unroll
                for (int k = 0; k < KD; ++k) { l[k] = __expf(l[k] - m); sum += l[k]; }
                v[0] = w * (m + __logf(sum) - lt);
                const float inv = 1.f / sum;
#pragma unroll
                for (int k = 0; k < KD; ++k) {
                    const float pk = l[k] * inv;
                    v[3 + k] = (k == t) ? pk : 0.f;
                    v[3 + KD + k] = pk;
                    v[3 + 2 * KD + k] = (k == t) ? 1.f : 0.f;
                }
            }
            v[1] = w;
        }
    }
    block_sum<NV>(v, red, partials + (size_t)blockIdx.x * NV);
}

// out = [loss, sum w (the pixel count without weights), bad targets, CE, Dice, a[N][KD], b[N][KD]]:
//   dDice / dp_ik = a_nk [t_i = k] + b_nk  on the valid pixels of image n (what the backward kernel needs from the sums)
// One workgroup; wave w sums the partial rows of images w, w + 4, .. in double (lanes stride the rows, then the cross-lane
// tree), thread 0 adds the four waves' totals in wave order.
template <int KD>
__global__ __launch_bounds__(MEDT_THREADS) void seg_loss_finalize_kernel(const float* __restrict__ partials,
                                                                         float* __restrict__ out, int N, int bpi,
                                                                         float ce_scale, float dice_scale, float eps) {
    constexpr int NV = 3 + 3 * KD;
    MEDT_STATIC_SHARED double tot[MEDT_WAVES * 4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double s_nll = 0.0, s_w = 0.0, s_bad = 0.0, s_dice = 0.0;
    for (int n = wave; n < N; n += MEDT_WAVES) {
        double acc[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) acc[j] = 0.0;
        for (int b = lane; b < bpi; b += 64) {
            const float* pp = partials + ((size_t)n * bpi + b) * NV;
#pragma unroll
            for (int j = 0; j < NV; ++j) acc[j] += (double)pp[j];
        }
#pragma unroll
        for (int j = 0; j < NV; ++j) acc[j] = wave_sum_d(acc[j]);
        s_nll += acc[0];
        s_w += acc[1];
        s_bad += acc[2];
        if constexpr (KD > 0) {
            const double nk = (double)N * KD;
#pragma unroll
            for (int k = 0; k < KD; ++k) {
                const double num = 2.0 * acc[3 + k] + (double)eps;
                const double D = acc[3 + KD + k] + acc[3 + 2 * KD + k] + (double)eps;
                s_dice += num / D;
                if (lane == 0) {
                    out[5 + (size_t)n * KD + k] = (float)(-2.0 / (D * nk));
                    out[5 + ((size_t)N + n) * KD + k] = (float)(num / (D * D * nk));
                }
            }
        }
    }
    if (lane == 0) {
        tot[wave * 4] = s_nll;
        tot[wave * 4 + 1] = s_w;
        tot[wave * 4 + 2] = s_bad;
        tot[wave * 4 + 3] = s_dice;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t[4] = {0.0, 0.0, 0.0, 0.0};
        for (int w = 0; w < MEDT_WAVES; ++w)
            for (int j = 0; j < 4; ++j) t[j] += tot[w * 4 + j];
        const double ce = t[0] / t[1];                              // no counted weight: 0/0 = NaN, as in torch
        double dice = 0.0;
        if constexpr (KD > 0) dice = 1.0 - t[3] / ((double)N * KD);
        double loss = 0.0;                                          // a switched-off term stays out (0 * NaN)
        if (ce_scale != 0.f) loss += (double)ce_scale * ce;
        if (dice_scale != 0.f) loss += (double)dice_scale * dice;
        out[0] = (float)loss;
        out[1] = (float)t[1];
        out[2] = (float)t[2];
        out[3] = (float)ce;
        out[4] = (float)dice;
    }
}

// dlogits[n,j,p] = dloss * ( ce_scale * w[t] / sum w * (p_j - [j == t])  +  dice_scale * p_j * (g_j - sum_k p_k g_k) ),
// g_k = a_nk [t == k] + b_nk;  pixels that are not valid get 0 in every class
template <int KD>
__global__ __launch_bounds__(MEDT_THREADS) void seg_loss_bwd_kernel(const float* __restrict__ logits,
                                                                    const int64_t* __restrict__ target,
                                                                    const float* __restrict__ weight,
                                                                    const float* __restrict__ out,
                                                                    const float* __restrict__ dloss,
                                                                    float* __restrict__ dlogits, int N, int K, int HW,
                                                                    int bpi, int ignore, float ce_scale, float dice_scale) {
    const int n = blockIdx.x / bpi;
    const int p = (blockIdx.x - n * bpi) * MEDT_THREADS + threadIdx.x;
    if (p >= HW) return;
    const int64_t t = target[(size_t)n * HW + p];
    const float* lp = logits + (size_t)n * K * HW + p;
    float* dp = dlogits + (size_t)n * K * HW + p;
    if (t == ignore || t < 0 || t >= K) {
        for (int k = 0; k < K; ++k) dp[(size_t)k * HW] = 0.f;
        return;
    }
    const float dl = dloss ? dloss[0] : 1.f;
    const float cs = ce_scale != 0.f ? ce_scale * (weight ? weight[t] : 1.f) / out[1] * dl : 0.f;
    if constexpr (KD == 0) {
        float m = lp[0];
        for (int k = 1; k < K; ++k) m = fmaxf(m, lp[(size_t)k * HW]);
        float sum = 0.f;
        for (int k = 0; k < K; ++k) sum += __expf(lp[(size_t)k * HW] - m);
        const float inv = 1.f / sum;
        for (int k = 0; k < K; ++k) {
            const float pk = __expf(lp[(size_t)k * HW] - m) * inv;
            dp[(size_t)k * HW] = (pk - (k == t ? 1.f : 0.f)) * cs;
        }
    } else {
        const float* ca = out + 5 + (size_t)n * KD;              // workgroup-uniform: one image per workgroup
        const float* cb = out + 5 + ((size_t)N + n) * KD;
        const float ds = dice_scale * dl;
        float l[KD], g[KD];
#pragma unroll
        for (int k = 0; k < KD; ++k) l[k] = lp[(size_t)k * HW];
        float m = l[0];
#pragma unroll
        for (int k = 1; k < KD; ++k) m = fmaxf(m, l[k]);
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < KD; ++k) { l[k] = __expf(l[k] - m); sum += l[k]; }
        const float inv = 1.f / sum;
        float dot = 0.f;
#pragma unroll
        for (int k = 0; k < KD; ++k) {
            l[k] *= inv;
            g[k] = ds * ((k == t ? ca[k] : 0.f) + cb[k]);
            dot += l[k] * g[k];
        }
#pragma unroll
        for (int k = 0; k < KD; ++k) dp[(size_t)k * HW] = l[k] * (g[k] - dot) + cs * (l[k] - (k == t ? 1.f : 0.f));
    }
}

int seg_loss_bpi(int HW) { return cdiv(HW, MEDT_THREADS); }
size_t seg_loss_partials(int N, int K, int HW) { return (size_t)N * seg_loss_bpi(HW) * (3 + (K <= 8 ? 3 * K : 0)); }
size_t seg_loss_out_floats(int N, int K) { return 5 + 2 * (size_t)N * K; }

// SEG_LOSS_KD(X): X(KD) for the instance that serves (K, Dice on or off)
#define SEG_LOSS_KD(X)                                                                                                 \
    switch (dice_scale != 0.f ? K : 0) {                                                                               \
        case 0: X(0); break;                                                                                           \
        case 2: X(2); break;                                                                                           \
        case 3: X(3); break;                                                                                           \
        case 4: X(4); break;                                                                                           \
        case 5: X(5); break;                                                                                           \
        case 6: X(6); break;                                                                                           \
        case 7: X(7); break;                                                                                           \
        case 8: X(8); break;                                                                                           \
        default: set_error("seg_loss: soft Dice needs 2 <= K <= 8 classes (K = %d)", K); return MEDT_EINVAL;           \
    }

int seg_loss_fwd(const float* logits, const int64_t* target, const float* weight, float* partials, float* out, int N, int K,
                 int HW, int ignore, float ce_scale, float dice_scale, float eps, hipStream_t s) {
    const int bpi = seg_loss_bpi(HW);
#define SEG_LOSS_FWD(KD)                                                                                               \
    hipLaunchKernelGGL(seg_loss_fwd_kernel<KD>, dim3((unsigned)N * bpi), dim3(MEDT_THREADS), 0, s, logits, target, weight, \
                       partials, K, HW, bpi, ignore)
    SEG_LOSS_KD(SEG_LOSS_FWD)
#undef SEG_LOSS_FWD
    int rc = launch_status("seg_loss_fwd");
    if (rc) return rc;
#define SEG_LOSS_FIN(KD)                                                                                               \
    hipLaunchKernelGGL(seg_loss_finalize_kernel<KD>, dim3(1), dim3(MEDT_THREADS), 0, s, partials, out, N, bpi, ce_scale, \
                       dice_scale, eps)
    SEG_LOSS_KD(SEG_LOSS_FIN)
#undef SEG_LOSS_FIN
    return launch_status("seg_loss_finalize");
}

int seg_loss_bwd(const float* logits, const int64_t* target, const float* weight, const float* out, const float* dloss,
                 float* dlogits, int N, int K, int HW, int ignore, float ce_scale, float dice_scale, hipStream_t s) {
    const int bpi = seg_loss_bpi(HW);
#define SEG_LOSS_BWD(KD)                                                                                               \
    hipLaunchKernelGGL(seg_loss_bwd_kernel<KD>, dim3((unsigned)N * bpi), dim3(MEDT_THREADS), 0, s, logits, target, weight, \
                       out, dloss, dlogits, N, K, HW, bpi, ignore, ce_scale, dice_scale)
    SEG_LOSS_KD(SEG_LOSS_BWD)
#undef SEG_LOSS_BWD
    return launch_status("seg_loss_bwd");
}
#undef SEG_LOSS_KD

// --------------------------------------------------------------------------- //
// AxialAttention_gated_sig (reference lib/models/model_codes.py:279-280, 292-293): the four gates enter through a sigmoid
// --------------------------------------------------------------------------- //
__global__ void gate_sigmoid_fwd_kernel(const float* f_qr, const float* f_kr, const float* f_sve, const float* f_sv,
                                        float* __restrict__ eff) {
    const float* src[4] = {f_qr, f_kr, f_sve, f_sv};
    const int k = threadIdx.x;
    if (k < 4) eff[k] = 1.f / (1.f + expf(-*src[k]));
}
__global__ void gate_sigmoid_bwd_kernel(const float* __restrict__ d_eff, const float* __restrict__ eff,
                                        float* __restrict__ dgate) {
    const int k = threadIdx.x;
    if (k < 4) dgate[k] = d_eff[k] * eff[k] * (1.f - eff[k]);
}
int gate_sigmoid_fwd(const float* f_qr, const float* f_kr, const float* f_sve, const float* f_sv, float* eff, hipStream_t s) {
    hipLaunchKernelGGL(gate_sigmoid_fwd_kernel, dim3(1), dim3(64), 0, s, f_qr, f_kr, f_sve, f_sv, eff);
    return launch_status("gate_sigmoid_fwd");
}
int gate_sigmoid_bwd(const float* d_eff, const float* eff, float* dgate, hipStream_t s) {
    hipLaunchKernelGGL(gate_sigmoid_bwd_kernel, dim3(1), dim3(64), 0, s, d_eff, eff, dgate);
    return launch_status("gate_sigmoid_bwd");
}

// --------------------------------------------------------------------------- //
// AxialAttention_gated_data (reference lib/models/model_codes.py:316-443): four gates PER SEQUENCE from a two-layer MLP
// on the sequence-averaged input (:371-380):  xn = mean_L x;  h = relu(W1 xn + b1);  o = relu(W2 h + b2);  s = sigmoid(o);
// gate columns (qr, kr, sv, sve) = s[:, 0..3] (:376-379, 406-407, 420-421).  One wave per sequence.
// --------------------------------------------------------------------------- //
__global__ __launch_bounds__(64) void gate_mlp_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w1,
                                                          const float* __restrict__ b1, const float* __restrict__ w2,
                                                          const float* __restrict__ b2, float* __restrict__ xn,
                                                          float* __restrict__ h, float* __restrict__ o,
                                                          float* __restrict__ gates, int C, int H, int W, int axis) {
    extern __shared__ float sm[];                      // xn[C] | h[C]
    const int b = blockIdx.x, Bo = axis ? H : W, L = axis ? W : H, n = b / Bo, sq = b - n * Bo, HW = H * W;
    const int pstride = axis ? 1 : W;
    for (int c = threadIdx.x; c < C; c += 64) {
        const float* p = x + ((size_t)n * C + c) * HW + (axis ? sq * W : sq);
        float a = 0.f;
        for (int i = 0; i < L; ++i) a += p[(size_t)i * pstride];
        a *= 1.f / (float)L;
        sm[c] = a;
        xn[(size_t)b * C + c] = a;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 64) {
        float a = b1[c];
        for (int k = 0; k < C; ++k) a = fmaf(w1[(size_t)c * C + k], sm[k], a);
        a = fmaxf(a, 0.f);
        sm[C + c] = a;
        h[(size_t)b * C + c] = a;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        float a = b2[threadIdx.x];
        for (int k = 0; k < C; ++k) a = fmaf(w2[threadIdx.x * C + k], sm[C + k], a);
        a = fmaxf(a, 0.f);
        o[b * 4 + threadIdx.x] = a;
        gates[b * 4 + threadIdx.x] = 1.f / (1.f + expf(-a));
    }
}

int gate_mlp_fwd(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, float* xn, float* h,
                 float* o, float* gates, int N, int C, int H, int W, int axis, hipStream_t s) {
    const int nseq = N * (axis ? H : W);
    hipLaunchKernelGGL(gate_mlp_fwd_kernel, dim3(nseq), dim3(64), 2 * C * sizeof(float), s, x, w1, b1, w2, b2, xn, h, o, gates,
                       C, H, W, axis);
    return launch_status("gate_mlp_fwd");
}

// per sequence: d_o = dgates * s(1-s) * [o > 0];  dh = (W2^T d_o) * [h > 0];  dxn = W1^T dh
__global__ __launch_bounds__(64) void gate_mlp_bwd_seq_kernel(const float* __restrict__ dgates, const float* __restrict__ gates,
                                                              const float* __restrict__ o, const float* __restrict__ h,
                                                              const float* __restrict__ w1, const float* __restrict__ w2,
                                                              float* __restrict__ d_o, float* __restrict__ dh,
                                                              float* __restrict__ dxn, int C) {
    extern __shared__ float sm[];                      // d_o[4] | dh[C]
    const int b = blockIdx.x;
    if (threadIdx.x < 4) {
        const float sg = gates[b * 4 + threadIdx.x];
        const float v = o[b * 4 + threadIdx.x] > 0.f ? dgates[b * 4 + threadIdx.x] * sg * (1.f - sg) : 0.f;
        sm[threadIdx.x] = v;
        d_o[b * 4 + threadIdx.x] = v;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 64) {
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) a = fmaf(w2[k * C + c], sm[k], a);
        a = h[(size_t)b * C + c] > 0.f ? a : 0.f;
        sm[4 + c] = a;
        dh[(size_t)b * C + c] = a;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 64) {
        float a = 0.f;
        for (int k = 0; k < C; ++k) a = fmaf(w1[(size_t)k * C + c], sm[4 + k], a);
        dxn[(size_t)b * C + c] = a;
    }
}

// parameter gradients (sums over the sequences): block r < C: row r of dW1 and db1[r]; block C + k: row k of dW2, db2[k]
__global__ __launch_bounds__(64) void gate_mlp_bwd_param_kernel(const float* __restrict__ d_o, const float* __restrict__ dh,
                                                                const float* __restrict__ h, const float* __restrict__ xn,
                                                                float* __restrict__ dw1, float* __restrict__ db1,
                                                                float* __restrict__ dw2, float* __restrict__ db2, int C,
                                                                int nseq) {
    const int r = blockIdx.x;
    const bool first = r < C;
    const int row = first ? r : r - C, stride = first ? C : 4;
    const float* lhs = first ? dh : d_o;                 // [b][row]
    const float* rhs = first ? xn : h;                   // [b][c]
    for (int c = threadIdx.x; c < C; c += 64) {
        float a = 0.f;
        for (int b = 0; b < nseq; ++b) a = fmaf(lhs[(size_t)b * stride + row], rhs[(size_t)b * C + c], a);
        (first ? dw1 : dw2)[(size_t)row * C + c] = a;
    }
    if (threadIdx.x == 0) {
        float a = 0.f;
        for (int b = 0; b < nseq; ++b) a += lhs[(size_t)b * stride + row];
        (first ? db1 : db2)[row] = a;
    }
}

// dx[n, c, pos] = dxn[b(n, pos), c] / L   (backward of the sequence mean)
__global__ __launch_bounds__(MEDT_THREADS) void gate_mlp_bwd_dx_kernel(const float* __restrict__ dxn, float* __restrict__ dx,
                                                                       int C, int H, int W, int axis, size_t total) {
    const size_t idx = (size_t)blockIdx.x * MEDT_THREADS + threadIdx.x;
    if (idx >= total) return;
    const int w = (int)(idx % W), hh = (int)((idx / W) % H), c = (int)((idx / ((size_t)W * H)) % C);
    const int n = (int)(idx / ((size_t)W * H * C));
    const int Bo = axis ? H : W, L = axis ? W : H, sq = axis ? hh : w;
    dx[idx] = dxn[((size_t)n * Bo + sq) * C + c] * (1.f / (float)L);
}

int gate_mlp_bwd(const float* dgates, const float* gates, const float* o, const float* h, const float* xn, const float* w1,
                 const float* w2, float* d_o, float* dh, float* dxn, float* dw1, float* db1, float* dw2, float* db2,
                 float* dx, int N, int C, int H, int W, int axis, hipStream_t s) {
    const int nseq = N * (axis ? H : W);
    hipLaunchKernelGGL(gate_mlp_bwd_seq_kernel, dim3(nseq), dim3(64), (4 + C) * sizeof(float), s, dgates, gates, o, h, w1, w2,
                       d_o, dh, dxn, C);
    int rc = launch_status("gate_mlp_bwd_seq");
    if (rc) return rc;
    hipLaunchKernelGGL(gate_mlp_bwd_param_kernel, dim3(C + 4), dim3(64), 0, s, d_o, dh, h, xn, dw1, db1, dw2, db2, C, nseq);
    if ((rc = launch_status("gate_mlp_bwd_param"))) return rc;
    const size_t total = (size_t)N * C * H * W;
    hipLaunchKernelGGL(gate_mlp_bwd_dx_kernel, dim3(grid1d(total)), dim3(MEDT_THREADS), 0, s, dxn, dx, C, H, W, axis, total);
    return launch_status("gate_mlp_bwd_dx");
}

// per-sequence gate gradients: sum over the heads, reorder (f_qr, f_kr, f_sve, f_sv) -> gate-tensor columns (qr, kr, sv, sve)
__global__ __launch_bounds__(MEDT_THREADS) void gate_seq_reduce_kernel(const float* __restrict__ partials,
                                                                       float* __restrict__ dgates, int nseq, int G) {
    const int idx = blockIdx.x * MEDT_THREADS + threadIdx.x;
    if (idx >= nseq * 4) return;
    const int b = idx >> 2, col = idx & 3, k = col == 2 ? 3 : (col == 3 ? 2 : col);
    float a = 0.f;
    for (int g = 0; g < G; ++g) a += partials[((size_t)b * G + g) * 4 + k];
    dgates[idx] = a;
}

int gate_seq_reduce(const float* partials, float* dgates, int nseq, int G, hipStream_t s) {
    hipLaunchKernelGGL(gate_seq_reduce_kernel, dim3(grid1d((size_t)nseq * 4)), dim3(MEDT_THREADS), 0, s, partials, dgates, nseq, G);
    return launch_status("gate_seq_reduce");
}

// --------------------------------------------------------------------------- //
// Adam (torch.optim.Adam semantics, coupled L2 weight decay).  The step counter lives on the device so a
// captured hipGraph replays correctly: adam_tick advances it and derives the bias corrections.
//   state[0] = step, state[1] = 1 - b1^step, state[2] = 1 - b2^step
// --------------------------------------------------------------------------- //
__global__ void adam_tick_kernel(float* __restrict__ state, float b1, float b2) {
    const float t = state[0] + 1.f;
    state[0] = t;
    state[1] = 1.f - powf(b1, t);
    state[2] = 1.f - powf(b2, t);
}

__global__ __launch_bounds__(MEDT_THREADS) void adam_step_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                                 float* __restrict__ m, float* __restrict__ v,
                                                                 const float* __restrict__ state, size_t n, float lr,
                                                                 float b1, float b2, float eps, float wd,
                                                                 float gscale) {
    const size_t i = (size_t)blockIdx.x * MEDT_THREADS + threadIdx.x;
    if (i >= n) return;
    const float bc1 = state[1], bc2 = state[2];
    const float pi = p[i];
    const float gi = fmaf(wd, pi, g[i] * gscale);
    const float mi = fmaf(b1, m[i], (1.f - b1) * gi);
    const float vi = fmaf(b2, v[i], (1.f - b2) * gi * gi);
    m[i] = mi;
    v[i] = vi;
    const float denom = sqrtf(vi) / sqrtf(bc2) + eps;
    p[i] = pi - (lr / bc1) * (mi / denom);
}

int adam_step(float* p, const float* g, float* m, float* v, float* state, size_t n, float lr, float b1, float b2,
              float eps, float wd, float gscale, hipStream_t s) {
    hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(1), 0, s, state, b1, b2);
    int rc = launch_status("adam_tick");
    if (rc) return rc;
    hipLaunchKernelGGL(adam_step_kernel, dim3(grid1d(n)), dim3(MEDT_THREADS), 0, s, p, g, m, v, state, n, lr, b1, b2, eps,
                       wd, gscale);
    return launch_status("adam_step");
}

// --------------------------------------------------------------------------- //
// Per-image confusion counts of a 2-class segmentation: prediction = logits[:,1] >= threshold (what test.py writes
// as PNG, test.py:131-137), ground truth = target > 0.  counts[n] = {tp, fp, fn, tn} (integer atomics: exact and
// order independent).  Replaces the per-pixel loops of performancemetrics_*.m.
// --------------------------------------------------------------------------- //
__global__ __launch_bounds__(MEDT_THREADS) void seg_counts_kernel(const float* __restrict__ logits,
                                                                  const int64_t* __restrict__ target,
                                                                  int* __restrict__ counts, int K, int HW,
                                                                  float threshold) {
    const int n = blockIdx.y;
    const float* fg = logits + ((size_t)n * K + 1) * HW;
    const int64_t* t = target + (size_t)n * HW;
    int tp = 0, fp = 0, fn = 0, tn = 0;
    for (int p = blockIdx.x * MEDT_THREADS + threadIdx.x; p < HW; p += gridDim.x * MEDT_THREADS) {
        const bool pred = fg[p] >= threshold, gt = t[p] > 0;
        tp += pred && gt;
        fp += pred && !gt;
        fn += !pred && gt;
        tn += !pred && !gt;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        tp += __shfl_xor(tp, o, 64);
        fp += __shfl_xor(fp, o, 64);
        fn += __shfl_xor(fn, o, 64);
        tn += __shfl_xor(tn, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(counts + n * 4 + 0, tp);
        atomicAdd(counts + n * 4 + 1, fp);
        atomicAdd(counts + n * 4 + 2, fn);
        atomicAdd(counts + n * 4 + 3, tn);
    }
}

// counts = 0 as a kernel, not a memset: captured behind a forward with parallel branches (InferStep), the memset node of the
// replayed graph did not reliably run between the forward's last kernel and the counting kernel -- test.py's score line came
// out of counts added to whatever an intermediate of the forward had left in that pool block.  Kernel after kernel is ordered.
__global__ __launch_bounds__(MEDT_THREADS) void seg_counts_zero_kernel(int* __restrict__ counts, int n) {
    const int i = blockIdx.x * MEDT_THREADS + threadIdx.x;
    if (i < n) counts[i] = 0;
}

int seg_counts(const float* logits, const int64_t* target, int* counts, int N, int K, int HW, float threshold,
               hipStream_t s) {
    hipLaunchKernelGGL(seg_counts_zero_kernel, dim3(cdiv(N * 4, MEDT_THREADS)), dim3(MEDT_THREADS), 0, s, counts, N * 4);
    if (int rc = launch_status("seg_counts_zero")) return rc;
    const int parts = min(cdiv(HW, MEDT_THREADS), 64);
    hipLaunchKernelGGL(seg_counts_kernel, dim3(parts, N), dim3(MEDT_THREADS), 0, s, logits, target, counts, K, HW, threshold);
    return launch_status("seg_counts");
}

// --------------------------------------------------------------------------- //
// Sliding-window inference on images larger than the network input (medt_amd/window.py): cut (C,H,W) into T = ny*nx
// overlapping S x S windows, and blend the T window logits back into one (K,H,W) map.  Window t = iy*nx + ix has its
// top-left corner at (oy[iy], ox[ix]); the origins are DEVICE arrays, so one launch geometry serves every plan of an
// image size.  Both kernels: a work-item is 4 consecutive x of one row, grid-stride loop, 16-byte stores when the
// destination rows are 16-byte aligned (VEC4), element stores otherwise.
// --------------------------------------------------------------------------- //
static inline unsigned grid_strided(size_t items) {
    return (unsigned)min((items + MEDT_THREADS - 1) / MEDT_THREADS, (size_t)4096);
}

// windows[t,c,i,j] = image[c, clamp(oy+i), clamp(ox+j)]: clamping to the image is the edge replication of an axis
// shorter than S (and keeps every read in bounds whatever the origin arrays hold)
template <bool VEC4>
__global__ __launch_bounds__(MEDT_THREADS) void window_gather_kernel(const float* __restrict__ image,
                                                                     float* __restrict__ windows,
                                                                     const int32_t* __restrict__ oy,
                                                                     const int32_t* __restrict__ ox, int C, int H, int W,
                                                                     int S, int nx, size_t items) {
    const int S4 = (S + 3) >> 2;
    for (size_t it = (size_t)blockIdx.x * MEDT_THREADS + threadIdx.x; it < items; it += (size_t)gridDim.x * MEDT_THREADS) {
        const int j0 = (int)(it % S4) * 4;
        size_t r = it / S4;
        const int i = (int)(r % S);
        r /= S;
        const int c = (int)(r % C), t = (int)(r / C);
        const int iy = t / nx, ix = t - iy * nx;
        const int y = min(max(oy[iy] + i, 0), H - 1), x0 = ox[ix] + j0;
        const float* src = image + ((size_t)c * H + y) * W;
        float* dst = windows + (((size_t)t * C + c) * S + i) * S + j0;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = src[min(max(x0 + e, 0), W - 1)];
        if (VEC4) {
            *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (j0 + e < S) dst[e] = v[e];
        }
    }
}

int window_gather(const float* image, float* windows, const int32_t* oy, const int32_t* ox, int C, int H, int W, int S,
                  int ny, int nx, hipStream_t s) {
    const size_t items = (size_t)ny * nx * C * S * ((S + 3) / 4);
    if ((S % 4 == 0) && ((uintptr_t)windows % 16 == 0))
        hipLaunchKernelGGL((window_gather_kernel<true>), dim3(grid_strided(items)), dim3(MEDT_THREADS), 0, s, image, windows,
                           oy, ox, C, H, W, S, nx, items);
    else
        hipLaunchKernelGGL((window_gather_kernel<false>), dim3(grid_strided(items)), dim3(MEDT_THREADS), 0, s, image, windows,
                           oy, ox, C, H, W, S, nx, items);
    return launch_status("window_gather");
}

// blended[k,y,x] = sum_t w_t l_t / sum_t w_t over the windows t that cover (y, x), w_t = w(y - oy) w(x - ox),
// w(i) = min(i + 1, S - i).  Gather form: the work-item owns its 4 pixels and visits the covering windows in the fixed
// order iy ascending, ix ascending inside -- no atomics, the same bits on every run.  A pixel covered by ONE window takes
// that window's value as it is (no (w l) / w round trip).  mask[y,x] = 255 (blended[1,y,x] >= threshold), written by the
// work-items of k = 1.  The covering rows / columns are located by one pass over oy and one over ox (first and last
// index whose window reaches the pixel); the test inside the loops makes the result right for any origin arrays.
template <bool VEC4>
__global__ __launch_bounds__(MEDT_THREADS) void window_blend_kernel(const float* __restrict__ win, float* __restrict__ blended,
                                                                    uint8_t* __restrict__ mask,
                                                                    const int32_t* __restrict__ oy,
                                                                    const int32_t* __restrict__ ox, int k0, int K,
                                                                    int H, int W, int S, int ny, int nx, float threshold,
                                                                    size_t items) {
    const int W4 = (W + 3) >> 2;
    for (size_t it = (size_t)blockIdx.x * MEDT_THREADS + threadIdx.x; it < items; it += (size_t)gridDim.x * MEDT_THREADS) {
        const int x0 = (int)(it % W4) * 4;
        const size_t r = it / W4;
        const int y = (int)(r % H), k = k0 + (int)(r / H);
        int iy_lo = ny, iy_hi = -1, ix_lo = nx, ix_hi = -1;
        for (int iy = 0; iy < ny; ++iy)
            if ((unsigned)(y - oy[iy]) < (unsigned)S) { iy_lo = min(iy_lo, iy); iy_hi = iy; }
        for (int ix = 0; ix < nx; ++ix) {
            const int d = x0 - ox[ix];                          // the window reaches one of x0 .. x0+3
            if (d > -4 && d < S) { ix_lo = min(ix_lo, ix); ix_hi = ix; }
        }
        float acc[4] = {0.f, 0.f, 0.f, 0.f}, wsum[4] = {0.f, 0.f, 0.f, 0.f}, one[4] = {0.f, 0.f, 0.f, 0.f};
        int n[4] = {0, 0, 0, 0};
        for (int iy = iy_lo; iy <= iy_hi; ++iy) {
            const int i = y - oy[iy];
            if ((unsigned)i >= (unsigned)S) continue;
            const float wy = (float)min(i + 1, S - i);
            for (int ix = ix_lo; ix <= ix_hi; ++ix) {
                const int d = x0 - ox[ix];
                if (d <= -4 || d >= S) continue;
                const float* row = win + ((((size_t)iy * nx + ix) * K + k) * S + i) * S;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int j = d + e;
                    if ((unsigned)j < (unsigned)S) {
                        const float l = row[j], w = wy * (float)min(j + 1, S - j);
                        acc[e] = fmaf(w, l, acc[e]);
                        wsum[e] += w;
                        one[e] = l;
                        ++n[e];
                    }
                }
            }
        }
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = n[e] == 1 ? one[e] : (n[e] ? acc[e] / wsum[e] : 0.f);
        const size_t px = (size_t)y * W + x0;
        if (VEC4) {
            if (blended) *reinterpret_cast<float4*>(blended + (size_t)k * H * W + px) = make_float4(v[0], v[1], v[2], v[3]);
            if (mask && k == 1) {
                uint32_t m = 0;                                   // 4 mask bytes as one 32-bit store (little endian)
#pragma unroll
                for (int e = 0; e < 4; ++e) m |= (v[e] >= threshold ? 255u : 0u) << (8 * e);
                *reinterpret_cast<uint32_t*>(mask + px) = m;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (x0 + e >= W) break;
                if (blended) blended[(size_t)k * H * W + px + e] = v[e];
                if (mask && k == 1) mask[px + e] = v[e] >= threshold ? 255 : 0;
            }
        }
    }
}

int window_blend(const float* win, float* blended, uint8_t* mask, const int32_t* oy, const int32_t* ox, int K, int H, int W,
                 int S, int ny, int nx, float threshold, hipStream_t s) {
    const int k0 = blended ? 0 : 1, nk = blended ? K : 1;       // mask only: the foreground channel alone
    const size_t items = (size_t)nk * H * ((W + 3) / 4);
    if ((W % 4 == 0) && ((uintptr_t)blended % 16 == 0) && ((uintptr_t)mask % 4 == 0))
        hipLaunchKernelGGL((window_blend_kernel<true>), dim3(grid_strided(items)), dim3(MEDT_THREADS), 0, s, win, blended, mask,
                           oy, ox, k0, K, H, W, S, ny, nx, threshold, items);
    else
        hipLaunchKernelGGL((window_blend_kernel<false>), dim3(grid_strided(items)), dim3(MEDT_THREADS), 0, s, win, blended,
                           mask, oy, ox, k0, K, H, W, S, ny, nx, threshold, items);
    return launch_status("window_blend");
}

// --------------------------------------------------------------------------- //
// Test-time augmentation at inference (medt_amd/tta.py; not in the reference): the eight views of the dihedral group of the
// square, numbered by a 3-bit code v -- bit 2 transpose, bit 1 flip rows, bit 0 flip columns (transpose first) -- and a set of
// views as a bitmask, visited in ascending code.
//   expand: x (N,C,H,W) -> out (N V,C,H,W), out[n V + j] = F_vj(x[n]), a bit copy;   F_v(a)[y,x] = a'[fy(y), fx(x)], a' = a or a^T
//   merge:  view logits (N V,K,H,W) -> the mean of the views mapped back, B_v(l)[y,x] = l[fy(y), fx(x)], or l[fy(x), fx(y)] with
//           bit 2, added in ascending code by the ONE work-item that owns the output element and divided by V once.
// Both kernels: a workgroup owns one TTA_T x TTA_T tile of one plane (expand: of the source, which it reads once for all views;
// merge: of the output), a work-item 4 consecutive x of one tile row.  The views without bit 2 are row copies, forwards or
// reversed, register to register.  The views with bit 2 go through an LDS tile of TTA_T + 1 floats per row, so that the global
// read and the global write both run along rows: the tile is written along its rows (bank = row + column mod 32, the 32 lanes of
// a half wave cover 4 rows x 8 quads: all distinct) and read along its columns (tile[q4 + e][i]: the same sum).  16-byte global
// accesses when W % 4 == 0 and the pointers are aligned (VEC4; a quad is then inside the plane or outside it as a whole, mirrored
// or not), element accesses with per-element bounds otherwise.  Tile edges are bounds, not a second kernel.
// --------------------------------------------------------------------------- //
constexpr int TTA_T = 32;
static_assert(MEDT_THREADS == TTA_T * (TTA_T / 4), "a work-item owns 4 neighbouring elements of a tile row");

// 4 elements of `row` starting at logical column c of a row of length W, the row mirrored when `flip`: e -> row[fx(c + e)]
template <bool VEC4>
__device__ __forceinline__ void tta_load4(const float* __restrict__ row, int c, int W, bool flip, float (&v)[4]) {
    if (VEC4) {
        if (c < W) {
            const float4 q = *reinterpret_cast<const float4*>(row + (flip ? W - 4 - c : c));
            if (flip) { v[0] = q.w; v[1] = q.z; v[2] = q.y; v[3] = q.x; } else { v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (c + e < W) v[e] = row[flip ? W - 1 - c - e : c + e];
    }
}

template <bool VEC4>
__device__ __forceinline__ void tta_store4(float* __restrict__ row, int c, int W, bool flip, const float (&v)[4]) {
    if (VEC4) {
        if (c < W)
            *reinterpret_cast<float4*>(row + (flip ? W - 4 - c : c)) =
                flip ? make_float4(v[3], v[2], v[1], v[0]) : make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (c + e < W) row[flip ? W - 1 - c - e : c + e] = v[e];
    }
}

template <bool VEC4>
__global__ __launch_bounds__(MEDT_THREADS) void tta_expand_kernel(const float* __restrict__ x, float* __restrict__ out, int C,
                                                                  int H, int W, unsigned views, int V, int tiles_x, int tiles) {
    MEDT_STATIC_SHARED float tile[TTA_T][TTA_T + 1];
    const int plane = blockIdx.x / tiles, tl = blockIdx.x - plane * tiles;
    const int ty = tl / tiles_x, tx = tl - ty * tiles_x;
    const int n = plane / C, c = plane - n * C;
    const int i = threadIdx.x >> 3, q4 = (threadIdx.x & 7) * 4;
    const int r0 = ty * TTA_T, c0 = tx * TTA_T;
    const size_t HW = (size_t)H * W;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    if (r0 + i < H) tta_load4<VEC4>(x + (size_t)plane * HW + (size_t)(r0 + i) * W, c0 + q4, W, false, a);
    if (views & 0xF0u) {                                    // (uniform: every work-item reaches the barrier)
#pragma unroll
        for (int e = 0; e < 4; ++e) tile[i][q4 + e] = a[e];
        __syncthreads();
    }
    int j = 0;
    for (int v = 0; v < 8; ++v) {
        if (!((views >> v) & 1u)) continue;
        float* dst = out + (((size_t)n * V + j) * C + c) * HW;
        ++j;
        const bool fr = (v & 2) != 0, fc = (v & 1) != 0;
        if (!(v & 4)) {                                     // source row r -> row fy(r), mirrored or not
            const int r = r0 + i;
            if (r < H) tta_store4<VEC4>(dst + (size_t)(fr ? H - 1 - r : r) * W, c0 + q4, W, fc, a);
        } else {                                            // H == W: source (r, s) -> out[fy(s)][fx(r)]; this work-item: s = c0 + i
            const int s = c0 + i;
            float t[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) t[e] = tile[q4 + e][i];
            if (s < W) tta_store4<VEC4>(dst + (size_t)(fr ? W - 1 - s : s) * W, r0 + q4, H, fc, t);
        }
    }
}

int tta_expand(const float* x, float* out, int N, int C, int H, int W, unsigned views, hipStream_t s) {
    const int V = __builtin_popcount(views), tiles_x = cdiv(W, TTA_T), tiles = tiles_x * cdiv(H, TTA_T);
    const dim3 grid((unsigned)((size_t)tiles * N * C)), block(MEDT_THREADS);
    if ((W % 4 == 0) && ((uintptr_t)x % 16 == 0) && ((uintptr_t)out % 16 == 0))
        hipLaunchKernelGGL((tta_expand_kernel<true>), grid, block, 0, s, x, out, C, H, W, views, V, tiles_x, tiles);
    else
        hipLaunchKernelGGL((tta_expand_kernel<false>), grid, block, 0, s, x, out, C, H, W, views, V, tiles_x, tiles);
    return launch_status("tta_expand");
}

// merged[n,k] = (B_v0(l_0) + B_v1(l_1) + ... ) / V, the additions in that order, one IEEE division (none for V = 1: the value
// passes through); mask = 255 (merged[n,1] >= threshold); votes = the number of views with their own l_j[n,1] >= threshold.
// The planes are k0 .. k0 + nk - 1 of every image: all K, or the foreground channel alone when merged is not asked for.
template <bool VEC4>
__global__ __launch_bounds__(MEDT_THREADS) void tta_merge_kernel(const float* __restrict__ lg, float* __restrict__ merged,
                                                                 uint8_t* __restrict__ mask, uint8_t* __restrict__ votes, int k0,
                                                                 int nk, int K, int H, int W, unsigned views, int V,
                                                                 float threshold, int tiles_x, int tiles) {
    MEDT_STATIC_SHARED float tile[TTA_T][TTA_T + 1];
    const int plane = blockIdx.x / tiles, tl = blockIdx.x - plane * tiles;
    const int ty = tl / tiles_x, tx = tl - ty * tiles_x;
    const int n = plane / nk, k = k0 + (plane - n * nk);
    const int i = threadIdx.x >> 3, q4 = (threadIdx.x & 7) * 4;
    const int y0 = ty * TTA_T, x0 = tx * TTA_T, y = y0 + i;
    const size_t HW = (size_t)H * W;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    int agree[4] = {0, 0, 0, 0};
    int j = 0;
    for (int v = 0; v < 8; ++v) {
        if (!((views >> v) & 1u)) continue;
        const float* src = lg + (((size_t)n * V + j) * K + k) * HW;
        const bool fr = (v & 2) != 0, fc = (v & 1) != 0;
        float l[4] = {0.f, 0.f, 0.f, 0.f};
        if (!(v & 4)) {
            if (y < H) tta_load4<VEC4>(src + (size_t)(fr ? H - 1 - y : y) * W, x0 + q4, W, fc, l);
        } else {
            // H == W.  B[y][x] = l[fy(x)][fx(y)]: stage tile[a][b] = l[fy(x0 + a)][fx(y0 + b)] by row reads (un-mirrored on the
            // way in), then this work-item's B[y0 + i][x0 + q4 + e] = tile[q4 + e][i]
            float t[4] = {0.f, 0.f, 0.f, 0.f};
            const int sx = x0 + i;
            if (sx < W) tta_load4<VEC4>(src + (size_t)(fr ? H - 1 - sx : sx) * W, y0 + q4, H, fc, t);
            __syncthreads();                                // the previous transposing view's readers are done
#pragma unroll
            for (int e = 0; e < 4; ++e) tile[i][q4 + e] = t[e];
            __syncthreads();
#pragma unroll
            for (int e = 0; e < 4; ++e) l[e] = tile[q4 + e][i];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            acc[e] = j == 0 ? l[e] : acc[e] + l[e];
            agree[e] += l[e] >= threshold ? 1 : 0;
        }
        ++j;
    }
    if (y >= H || x0 + q4 >= W) return;
    if (V > 1) {
        const float fv = (float)V;
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = acc[e] / fv;
    }
    const size_t px = (size_t)y * W + x0 + q4;
    if (merged) tta_store4<VEC4>(merged + ((size_t)n * K + k) * HW + (size_t)y * W, x0 + q4, W, false, acc);
    if (k != 1) return;
    if (VEC4) {
        uint32_t m = 0, a = 0;                              // 4 bytes as one 32-bit store (little endian)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            m |= (acc[e] >= threshold ? 255u : 0u) << (8 * e);
            a |= (uint32_t)agree[e] << (8 * e);
        }
        if (mask) *reinterpret_cast<uint32_t*>(mask + (size_t)n * HW + px) = m;
        if (votes) *reinterpret_cast<uint32_t*>(votes + (size_t)n * HW + px) = a;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (x0 + q4 + e >= W) break;
            if (mask) mask[(size_t)n * HW + px + e] = acc[e] >= threshold ? 255 : 0;
            if (votes) votes[(size_t)n * HW + px + e] = (uint8_t)agree[e];
        }
    }
}

int tta_merge(const float* view_logits, float* merged, uint8_t* mask, uint8_t* votes, int N, int K, int H, int W, unsigned views,
              float threshold, hipStream_t s) {
    const int V = __builtin_popcount(views), tiles_x = cdiv(W, TTA_T), tiles = tiles_x * cdiv(H, TTA_T);
    const int k0 = merged ? 0 : 1, nk = merged ? K : 1;         // mask / votes only: the foreground channel alone
    const dim3 grid((unsigned)((size_t)tiles * N * nk)), block(MEDT_THREADS);
    if ((W % 4 == 0) && ((uintptr_t)view_logits % 16 == 0) && ((uintptr_t)merged % 16 == 0) && ((uintptr_t)mask % 4 == 0) &&
        ((uintptr_t)votes % 4 == 0))
        hipLaunchKernelGGL((tta_merge_kernel<true>), grid, block, 0, s, view_logits, merged, mask, votes, k0, nk, K, H, W, views,
                           V, threshold, tiles_x, tiles);
    else
        hipLaunchKernelGGL((tta_merge_kernel<false>), grid, block, 0, s, view_logits, merged, mask, votes, k0, nk, K, H, W, views,
                           V, threshold, tiles_x, tiles);
    return launch_status("tta_merge");
}

// --------------------------------------------------------------------------- //
// Joint augmentation of a training batch on the device (medt_amd/augment.py; reference utils.py:70-98 does it per item
// with torchvision on the host): uint8 HWC images (N,H,W,C) + uint8 masks (N,H,W) -> float32 (N,C,th,tw) in [0,1] and
// int64 (N,th,tw).  One record of AUG_P floats per image, drawn on the host and kept in a DEVICE table, so one launch
// geometry serves every draw:
//   [0] cy  [1] cx  crop origin          [2] flip != 0          [3] identity != 0: no affine step
//   [4..9]  m00 m01 m02 m10 m11 m12      inverse affine map, output pixel centre -> cropped image
//   [10..13] operation of jitter slot k  0 none, 1 brightness, 2 contrast, 3 saturation, 4 hue
//   [14..17] factor of jitter slot k     [18..19] reserved, 0
// Output pixel (i, j):  (fx, fy) = m (j + .5, i + .5);  outside [0,tw) x [0,th) -- tested on the FLOATS, so NaN / huge
// coordinates are outside -- the image gets 0 and the mask class 0;  sx = floor(fx) (mirrored when flipped), sy = floor(fy);
// source pixel (cy + sy, cx + sx), clamped to the input like window_gather (no table makes a read leave the input);
// v = u8 / 255 (IEEE division: to_tensor's bits), then the jitter slots in order -- torchvision's float path.
// The source offset (cy*W + cx)*C is arbitrary, so the C bytes of a pixel are fetched as bytes: a 4-pixel identity run of
// 12 bytes is dword aligned for one origin in four, and neighbouring lanes' bytes share cache lines either way.
// --------------------------------------------------------------------------- //
constexpr int AUG_P = 20;
constexpr int AUG_CY = 0, AUG_CX = 1, AUG_FLIP = 2, AUG_IDENT = 3, AUG_M = 4, AUG_OP = 10, AUG_FAC = 14;
constexpr float AUG_BRIGHTNESS = 1.f, AUG_CONTRAST = 2.f, AUG_SATURATION = 3.f, AUG_HUE = 4.f;

size_t augment_param_floats() { return AUG_P; }
int augment_parts(int th, int tw) { return (int)min(((size_t)th * tw + 1023) / 1024, (size_t)32); }

__device__ __forceinline__ float aug_clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }

template <int C>
__device__ __forceinline__ float aug_gray(const float (&v)[C]) {
    if (C == 3) return 0.299f * v[0] + 0.587f * v[1 % C] + 0.114f * v[2 % C];      // channels AS STORED (BGR handed over as RGB)
    return v[0];
}

// torchvision.transforms.functional_tensor: _rgb2hsv, h = (h + hf) mod 1, _hsv2rgb (hexcone)
__device__ __forceinline__ void aug_hue(float (&v)[3], float hf) {
    const float r = v[0], g = v[1], b = v[2];
    const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
    const bool eqc = maxc == minc;
    const float cr = maxc - minc;
    const float s = cr / (eqc ? 1.f : maxc);
    const float crd = eqc ? 1.f : cr;
    const float rc = (maxc - r) / crd, gc = (maxc - g) / crd, bc = (maxc - b) / crd;
    float h = maxc == r ? bc - gc : (maxc == g ? 2.f + rc - bc : 4.f + gc - rc);
    h = fmodf(h / 6.f + 1.f, 1.f);
    h += hf;
    h -= floorf(h);
    const float h6 = h * 6.f, fi = floorf(h6), f = h6 - fi;
    const int i = (fi >= 0.f && fi < 7.f) ? (int)fi % 6 : 0;
    const float p = aug_clamp01(maxc * (1.f - s)), q = aug_clamp01(maxc * (1.f - s * f)),
                t = aug_clamp01(maxc * (1.f - s * (1.f - f)));
    switch (i) {
        case 0: v[0] = maxc; v[1] = t; v[2] = p; break;
        case 1: v[0] = q; v[1] = maxc; v[2] = p; break;
        case 2: v[0] = p; v[1] = maxc; v[2] = t; break;
        case 3: v[0] = p; v[1] = q; v[2] = maxc; break;
        case 4: v[0] = t; v[1] = p; v[2] = maxc; break;
        default: v[0] = maxc; v[1] = p; v[2] = q; break;
    }
}
__device__ __forceinline__ void aug_hue(float (&)[1], float) {}

// the jitter slots of one record on one pixel.  UNTIL_CONTRAST: stop in front of the first contrast slot and say whether
// there is one (augment_stats: mean_g is the mean grey of the image at that point)
template <int C, bool UNTIL_CONTRAST>
__device__ __forceinline__ bool aug_jitter(float (&v)[C], const float* __restrict__ rec, float mean_g) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float op = rec[AUG_OP + k], fac = rec[AUG_FAC + k];
        if (op == AUG_BRIGHTNESS) {
#pragma unroll
            for (int c = 0; c < C; ++c) v[c] = aug_clamp01(fac * v[c]);
        } else if (op == AUG_CONTRAST) {
            if (UNTIL_CONTRAST) return true;
#pragma unroll
            for (int c = 0; c < C; ++c) v[c] = aug_clamp01(fac * v[c] + (1.f - fac) * mean_g);
        } else if (op == AUG_SATURATION) {
            if (C == 3) {
                const float g = aug_gray<C>(v);
#pragma unroll
                for (int c = 0; c < C; ++c) v[c] = aug_clamp01(fac * v[c] + (1.f - fac) * g);
            }
        } else if (op == AUG_HUE) {
            aug_hue(v, fac);
        }
    }
    return false;
}

struct AugCrop {
    int cy, cx;
};
// the origin as integers inside the input, whatever the table holds (fmaxf(NaN, 0) = 0)
__device__ __forceinline__ AugCrop aug_origin(const float* __restrict__ rec, int H, int W) {
    AugCrop o;
    o.cy = (int)fminf(fmaxf(rec[AUG_CY], 0.f), (float)(H - 1));
    o.cx = (int)fminf(fmaxf(rec[AUG_CX], 0.f), (float)(W - 1));
    return o;
}

// partials[n][part] = sum of the grey value, in front of the record's contrast slot, over the part's share of the CROPPED
// th x tw image (0 when the record has no contrast).  Fixed order: a thread's pixels ascending, the xor tree of the wave,
// the four waves ascending; augment_apply adds the parts ascending.  No atomics.
template <int C>
__global__ __launch_bounds__(MEDT_THREADS) void augment_stats_kernel(const uint8_t* __restrict__ image,
                                                                     const float* __restrict__ params,
                                                                     float* __restrict__ partials, int H, int W, int th,
                                                                     int tw, int parts) {
    MEDT_STATIC_SHARED float red[MEDT_WAVES];
    const int n = blockIdx.y, part = blockIdx.x, tid = threadIdx.x;
    const float* rec = params + (size_t)n * AUG_P;
    const AugCrop o = aug_origin(rec, H, W);
    const int total = th * tw, chunk = (total + parts - 1) / parts;
    const int p1 = min(total, (part + 1) * chunk);
    float sum = 0.f;
    for (int p = part * chunk + tid; p < p1; p += MEDT_THREADS) {
        const int i = p / tw, j = p - i * tw;
        const int y = min(o.cy + i, H - 1), x = min(o.cx + j, W - 1);
        const uint8_t* src = image + (((size_t)n * H + y) * W + x) * C;
        float v[C];
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = (float)src[c] / 255.f;
        if (aug_jitter<C, true>(v, rec, 0.f)) sum += aug_gray<C>(v);
    }
    sum = wave_sum(sum);
    if ((tid & 63) == 0) red[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < MEDT_WAVES; ++w) s += red[w];
        partials[(size_t)n * parts + part] = s;
    }
}

struct alignas(16) AugLabel2 {
    int64_t a, b;
};

// a work-item: 4 consecutive output x of one row of image blockIdx.y, all channels.  means (N floats behind the partials)
// receives the mean grey the contrast slot used, 0 without statistics.
template <int C, bool VEC4>
__global__ __launch_bounds__(MEDT_THREADS) void augment_apply_kernel(const uint8_t* __restrict__ image,
                                                                     const uint8_t* __restrict__ mask,
                                                                     const float* __restrict__ params,
                                                                     const float* __restrict__ partials,
                                                                     float* __restrict__ means,
                                                                     float* __restrict__ out_image,
                                                                     int64_t* __restrict__ out_mask, int H, int W, int th,
                                                                     int tw, int parts, int items) {
    const int n = blockIdx.y;
    const float* rec = params + (size_t)n * AUG_P;
    const AugCrop o = aug_origin(rec, H, W);
    const bool flip = rec[AUG_FLIP] != 0.f, ident = rec[AUG_IDENT] != 0.f;
    const float m00 = rec[AUG_M], m01 = rec[AUG_M + 1], m02 = rec[AUG_M + 2], m10 = rec[AUG_M + 3], m11 = rec[AUG_M + 4],
                m12 = rec[AUG_M + 5];
    float mean_g = 0.f;
    if (partials) {
        double s = 0.0;
        for (int p = 0; p < parts; ++p) s += (double)partials[(size_t)n * parts + p];
        mean_g = (float)(s / (double)((size_t)th * tw));
    }
    if (means && blockIdx.x == 0 && threadIdx.x == 0) means[n] = mean_g;
    const int tw4 = (tw + 3) >> 2;
    for (int it = blockIdx.x * MEDT_THREADS + threadIdx.x; it < items; it += gridDim.x * MEDT_THREADS) {
        const int i = it / tw4, j0 = (it - i * tw4) * 4;
        float v[4][C];
        int64_t lab[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = j0 + e;
            int sx = j, sy = i;
            bool inside = VEC4 || j < tw;
            if (!ident) {
                const float fx = m00 * (j + 0.5f) + m01 * (i + 0.5f) + m02, fy = m10 * (j + 0.5f) + m11 * (i + 0.5f) + m12;
                inside = inside && fx >= 0.f && fx < (float)tw && fy >= 0.f && fy < (float)th;      // false for NaN
                sx = inside ? (int)floorf(fx) : 0;
                sy = inside ? (int)floorf(fy) : 0;
            }
            if (flip) sx = tw - 1 - sx;
            const int y = min(max(o.cy + sy, 0), H - 1), x = min(max(o.cx + sx, 0), W - 1);
            const size_t px = ((size_t)n * H + y) * W + x;
            lab[e] = 0;
#pragma unroll
            for (int c = 0; c < C; ++c) v[e][c] = 0.f;
            if (inside) {
                lab[e] = (int64_t)mask[px];
#pragma unroll
                for (int c = 0; c < C; ++c) v[e][c] = (float)image[px * C + c] / 255.f;
                aug_jitter<C, false>(v[e], rec, mean_g);
            }
        }
        int64_t* ml = out_mask + ((size_t)n * th + i) * tw + j0;
        if (VEC4) {
            AugLabel2 l01, l23;
            l01.a = lab[0]; l01.b = lab[1]; l23.a = lab[2]; l23.b = lab[3];
            reinterpret_cast<AugLabel2*>(ml)[0] = l01;
            reinterpret_cast<AugLabel2*>(ml)[1] = l23;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (j0 + e < tw) ml[e] = lab[e];
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float* dst = out_image + (((size_t)n * C + c) * th + i) * tw + j0;
            if (VEC4) {
                *reinterpret_cast<float4*>(dst) = make_float4(v[0][c], v[1][c], v[2][c], v[3][c]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (j0 + e < tw) dst[e] = v[e][c];
            }
        }
    }
}

int augment_stats(const uint8_t* image, const float* params, float* workspace, int N, int H, int W, int C, int th, int tw,
                  hipStream_t s) {
    const int parts = augment_parts(th, tw);
    if (C == 3)
        hipLaunchKernelGGL((augment_stats_kernel<3>), dim3(parts, N), dim3(MEDT_THREADS), 0, s, image, params, workspace, H, W,
                           th, tw, parts);
    else
        hipLaunchKernelGGL((augment_stats_kernel<1>), dim3(parts, N), dim3(MEDT_THREADS), 0, s, image, params, workspace, H, W,
                           th, tw, parts);
    return launch_status("augment_stats");
}

int augment_apply(const uint8_t* image, const uint8_t* mask, const float* params, float* workspace, float* out_image,
                  int64_t* out_mask, int N, int H, int W, int C, int th, int tw, int use_stats, hipStream_t s) {
    const int parts = augment_parts(th, tw), items = th * ((tw + 3) / 4);
    const float* partials = (workspace && use_stats) ? workspace : nullptr;
    float* means = workspace ? workspace + (size_t)N * parts : nullptr;
    const dim3 grid((unsigned)min((items + MEDT_THREADS - 1) / MEDT_THREADS, 1024), N), block(MEDT_THREADS);
    const bool vec = (tw % 4 == 0) && ((uintptr_t)out_image % 16 == 0) && ((uintptr_t)out_mask % 16 == 0);
#define MEDT_AUG_LAUNCH(CC, VV)                                                                                            \
    hipLaunchKernelGGL((augment_apply_kernel<CC, VV>), grid, block, 0, s, image, mask, params, partials, means, out_image, \
                       out_mask, H, W, th, tw, parts, items)
    if (C == 3) {
        if (vec) MEDT_AUG_LAUNCH(3, true); else MEDT_AUG_LAUNCH(3, false);
    } else {
        if (vec) MEDT_AUG_LAUNCH(1, true); else MEDT_AUG_LAUNCH(1, false);
    }
#undef MEDT_AUG_LAUNCH
    return launch_status("augment_apply");
}

// --------------------------------------------------------------------------- //
// Elastic deformation inside the joint augmentation (U-Net's "random displacement vectors on a coarse grid"; not in the
// reference): record slot [18] != 0 gives the image a cubic B-spline free-form deformation over G x G cells, 1 <= G <= 8.
// field (N,2,G+3,G+3) float32 is the control lattice in pixels, channel 0 = dx, channel 1 = dy, a DEVICE table.
// Output pixel (i, j) of a flagged record:
//   tx = (j+.5) G / tw, cx = min(floor(tx), G-1), u = tx - cx;  ty, cy, v likewise from i, th
//   B0 = (1-u)^3/6, B1 = (3u^3-6u^2+4)/6, B2 = (-3u^3+3u^2+3u+1)/6, B3 = u^3/6      (>= 0, sum 1)
//   d = sum_a B_a(v) (sum_b B_b(u) field[.][cy+a][cx+b]), b ascending inside, a ascending outside
//   p = (j+.5+dx, i+.5+dy);  f = M p, or p when the record has the identity flag;  inside as in augment_apply
//   mask: nearest, floor(f).  image: bilinear about pixel centres, ux = fx-.5, x0 = floor(ux), wx = ux-x0, taps x0, x0+1
//   clamped to the crop, mirrored when flipped, offset by the origin and clamped to the input; every tap is u8/255 and runs
//   through the jitter slots BEFORE the blend (1-wy)((1-wx) t00 + wx t01) + wy((1-wx) t10 + wx t11).
// A zero lattice under the identity flag has wx = wy = 0 exactly: the bits of augment_apply -- as long as aug_jitter, which is
// compiled with the default contraction, is contracted here as it is there: the tap loop therefore holds the 4 pixels in the
// shape augment_apply_kernel has them.  A record without the flag takes augment_apply's body (the flag is
// uniform over a block).  The spline, the map and the weights are evaluated without
// contraction, operation for operation as written, so the float32 restatement in tests/elastic_oracle.py follows them.
// Lattice indices are clamped to [0, G+2], tap indices as above: no table, finite or not, makes a read leave its buffer.
// --------------------------------------------------------------------------- //
constexpr int AUG_ELASTIC = 18, AUG_GMAX = 8, AUG_LMAX = AUG_GMAX + 3;

// the four cubic B-spline weights at u in [0, 1]
__device__ __forceinline__ void aug_bspline(float u, float (&B)[4]) {
#pragma clang fp contract(off)
    const float om = 1.f - u, u2 = u * u, u3 = u2 * u;
    B[0] = om * om * om / 6.f;
    B[1] = (3.f * u3 - 6.f * u2 + 4.f) / 6.f;
    B[2] = (-3.f * u3 + 3.f * u2 + 3.f * u + 1.f) / 6.f;
    B[3] = u3 / 6.f;
}

// cell and weights of output coordinate k of `extent` under a grid of G cells
__device__ __forceinline__ int aug_cell(int k, int extent, int G, float (&B)[4]) {
#pragma clang fp contract(off)
    const float t = (k + 0.5f) * (float)G / (float)extent;
    const int c = min(max((int)floorf(t), 0), G - 1);
    aug_bspline(t - (float)c, B);
    return c;
}

// the 4 pixels of a work-item to both outputs, as augment_apply_kernel stores them
template <int C, bool VEC4>
__device__ __forceinline__ void aug_store(const float (&v)[4][C], const int64_t (&lab)[4], float* __restrict__ out_image,
                                          int64_t* __restrict__ out_mask, int n, int i, int j0, int th, int tw) {
    int64_t* ml = out_mask + ((size_t)n * th + i) * tw + j0;
    if (VEC4) {
        AugLabel2 l01, l23;
        l01.a = lab[0]; l01.b = lab[1]; l23.a = lab[2]; l23.b = lab[3];
        reinterpret_cast<AugLabel2*>(ml)[0] = l01;
        reinterpret_cast<AugLabel2*>(ml)[1] = l23;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (j0 + e < tw) ml[e] = lab[e];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        float* dst = out_image + (((size_t)n * C + c) * th + i) * tw + j0;
        if (VEC4) {
            *reinterpret_cast<float4*>(dst) = make_float4(v[0][c], v[1][c], v[2][c], v[3][c]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (j0 + e < tw) dst[e] = v[e][c];
        }
    }
}

// a work-item: 4 consecutive output x of one row of image blockIdx.y, all channels, like augment_apply_kernel
template <int C, bool VEC4>
__global__ __launch_bounds__(MEDT_THREADS) void augment_warp_kernel(const uint8_t* __restrict__ image,
                                                                    const uint8_t* __restrict__ mask,
                                                                    const float* __restrict__ params,
                                                                    const float* __restrict__ field, int G,
                                                                    const float* __restrict__ partials,
                                                                    float* __restrict__ means,
                                                                    float* __restrict__ out_image,
                                                                    int64_t* __restrict__ out_mask, int H, int W, int th,
                                                                    int tw, int parts, int items) {
    MEDT_STATIC_SHARED float lat[2 * AUG_LMAX * AUG_LMAX];
    const int n = blockIdx.y;
    const float* rec = params + (size_t)n * AUG_P;
    const AugCrop o = aug_origin(rec, H, W);
    const bool flip = rec[AUG_FLIP] != 0.f, ident = rec[AUG_IDENT] != 0.f, elastic = rec[AUG_ELASTIC] != 0.f;
    const float m00 = rec[AUG_M], m01 = rec[AUG_M + 1], m02 = rec[AUG_M + 2], m10 = rec[AUG_M + 3], m11 = rec[AUG_M + 4],
                m12 = rec[AUG_M + 5];
    float mean_g = 0.f;
    if (partials) {
        double s = 0.0;
        for (int p = 0; p < parts; ++p) s += (double)partials[(size_t)n * parts + p];
        mean_g = (float)(s / (double)((size_t)th * tw));
    }
    if (means && blockIdx.x == 0 && threadIdx.x == 0) means[n] = mean_g;
    const int tw4 = (tw + 3) >> 2, L = G + 3, LL = L * L;
    if (!elastic) {                        // uniform over the block: augment_apply_kernel's body
        for (int it = blockIdx.x * MEDT_THREADS + threadIdx.x; it < items; it += gridDim.x * MEDT_THREADS) {
            const int i = it / tw4, j0 = (it - i * tw4) * 4;
            float v[4][C];
            int64_t lab[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int j = j0 + e;
                int sx = j, sy = i;
                bool inside = VEC4 || j < tw;
                if (!ident) {
                    const float fx = m00 * (j + 0.5f) + m01 * (i + 0.5f) + m02, fy = m10 * (j + 0.5f) + m11 * (i + 0.5f) + m12;
                    inside = inside && fx >= 0.f && fx < (float)tw && fy >= 0.f && fy < (float)th;      // false for NaN
                    sx = inside ? (int)floorf(fx) : 0;
                    sy = inside ? (int)floorf(fy) : 0;
                }
                if (flip) sx = tw - 1 - sx;
                const int y = min(max(o.cy + sy, 0), H - 1), x = min(max(o.cx + sx, 0), W - 1);
                const size_t px = ((size_t)n * H + y) * W + x;
                lab[e] = 0;
#pragma unroll
                for (int c = 0; c < C; ++c) v[e][c] = 0.f;
                if (inside) {
                    lab[e] = (int64_t)mask[px];
#pragma unroll
                    for (int c = 0; c < C; ++c) v[e][c] = (float)image[px * C + c] / 255.f;
                    aug_jitter<C, false>(v[e], rec, mean_g);
                }
            }
            aug_store<C, VEC4>(v, lab, out_image, out_mask, n, i, j0, th, tw);
        }
    } else {
        for (int k = threadIdx.x; k < 2 * LL; k += MEDT_THREADS) lat[k] = field[(size_t)n * 2 * LL + k];      // once per block
        __syncthreads();
        const float e00 = ident ? 1.f : m00, e01 = ident ? 0.f : m01, e02 = ident ? 0.f : m02, e10 = ident ? 0.f : m10,
                    e11 = ident ? 1.f : m11, e12 = ident ? 0.f : m12;
        const uint8_t* mask_n = mask + (size_t)n * H * W;
        for (int it = blockIdx.x * MEDT_THREADS + threadIdx.x; it < items; it += gridDim.x * MEDT_THREADS) {
            const int i = it / tw4, j0 = (it - i * tw4) * 4;
            float v[4][C];
            int64_t lab[4];
            float fx[4], fy[4];
            {                                                   // the geometry of the 4 pixels: spline, map
#pragma clang fp contract(off)
                float Bv[4];
                const int cy = aug_cell(i, th, G, Bv);          // row-uniform
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float Bu[4];
                    const int cx = aug_cell(j0 + e, tw, G, Bu);
                    float d[2];
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        float acc = 0.f;
#pragma unroll
                        for (int a = 0; a < 4; ++a) {
                            const float* row = lat + k * LL + min(max(cy + a, 0), L - 1) * L;
                            float s = 0.f;
#pragma unroll
                            for (int b = 0; b < 4; ++b) s = s + Bu[b] * row[min(max(cx + b, 0), L - 1)];
                            acc = acc + Bv[a] * s;
                        }
                        d[k] = acc;
                    }
                    const float px = (j0 + e + 0.5f) + d[0], py = (i + 0.5f) + d[1];
                    fx[e] = e00 * px + e01 * py + e02;          // (the identity flag: 1 px + 0 py + 0, px itself or NaN)
                    fy[e] = e10 * px + e11 * py + e12;
                }
            }
            bool inside[4];
            float wx[4], wy[4];
            int x0[4], y0[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {                       // the mask tap, the image taps' corner and weights
                inside[e] = (VEC4 || j0 + e < tw) && fx[e] >= 0.f && fx[e] < (float)tw && fy[e] >= 0.f && fy[e] < (float)th;   // false for NaN
                lab[e] = 0;
                wx[e] = wy[e] = 0.f;
                x0[e] = y0[e] = 0;
#pragma unroll
                for (int c = 0; c < C; ++c) v[e][c] = 0.f;
                if (inside[e]) {
#pragma clang fp contract(off)
                    int sx = (int)floorf(fx[e]);
                    const int sy = (int)floorf(fy[e]);
                    if (flip) sx = tw - 1 - sx;
                    const int my = min(max(o.cy + sy, 0), H - 1), mx = min(max(o.cx + sx, 0), W - 1);
                    lab[e] = (int64_t)mask_n[(size_t)my * W + mx];
                    const float ux = fx[e] - 0.5f, uy = fy[e] - 0.5f, fx0 = floorf(ux), fy0 = floorf(uy);
                    wx[e] = ux - fx0; wy[e] = uy - fy0;
                    x0[e] = (int)fx0; y0[e] = (int)fy0;
                }
            }
            float r[4][C];
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int c = 0; c < C; ++c) r[e][c] = 0.f;
#pragma unroll 1
            for (int tap = 0; tap < 4; ++tap) {                 // one tap at a time: fetch as bytes, jitter, blend
                const bool right = tap & 1, lower = tap >> 1;
                asm volatile("" ::: "memory");                  // the record is re-read per tap, where the jitter uses it (below)
                float t[4][C];
#pragma unroll
                for (int e = 0; e < 4; ++e) {                   // the 4 pixels side by side, as augment_apply_kernel has them
                    int sx = min(max(x0[e] + (int)right, 0), tw - 1);
                    const int sy = min(max(y0[e] + (int)lower, 0), th - 1);
                    if (flip) sx = tw - 1 - sx;
                    const int y = min(max(o.cy + sy, 0), H - 1), x = min(max(o.cx + sx, 0), W - 1);
                    const size_t px = ((size_t)n * H + y) * W + x;
#pragma unroll
                    for (int c = 0; c < C; ++c) t[e][c] = 0.f;
                    if (inside[e]) {
#pragma unroll
                        for (int c = 0; c < C; ++c) t[e][c] = (float)image[px * C + c] / 255.f;
                        aug_jitter<C, false>(t[e], rec, mean_g);
                    }
                }
                {
#pragma clang fp contract(off)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float wxk = right ? wx[e] : 1.f - wx[e], wyk = lower ? wy[e] : 1.f - wy[e];
#pragma unroll
                        for (int c = 0; c < C; ++c) {
                            r[e][c] = right ? r[e][c] + wxk * t[e][c] : wxk * t[e][c];
                            if (right) v[e][c] = lower ? v[e][c] + wyk * r[e][c] : wyk * r[e][c];
                        }
                    }
                }
            }
            aug_store<C, VEC4>(v, lab, out_image, out_mask, n, i, j0, th, tw);
        }
    }
}

int augment_warp(const uint8_t* image, const uint8_t* mask, const float* params, const float* field, int G, float* workspace,
                 float* out_image, int64_t* out_mask, int N, int H, int W, int C, int th, int tw, int use_stats, hipStream_t s) {
    const int parts = augment_parts(th, tw), items = th * ((tw + 3) / 4);
    const float* partials = (workspace && use_stats) ? workspace : nullptr;
    float* means = workspace ? workspace + (size_t)N * parts : nullptr;
    const dim3 grid((unsigned)min((items + MEDT_THREADS - 1) / MEDT_THREADS, 1024), N), block(MEDT_THREADS);
    const bool vec = (tw % 4 == 0) && ((uintptr_t)out_image % 16 == 0) && ((uintptr_t)out_mask % 16 == 0);
#define MEDT_AUG_LAUNCH(CC, VV)                                                                                          \
    hipLaunchKernelGGL((augment_warp_kernel<CC, VV>), grid, block, 0, s, image, mask, params, field, G, partials, means, \
                       out_image, out_mask, H, W, th, tw, parts, items)
    if (C == 3) {
        if (vec) MEDT_AUG_LAUNCH(3, true); else MEDT_AUG_LAUNCH(3, false);
    } else {
        if (vec) MEDT_AUG_LAUNCH(1, true); else MEDT_AUG_LAUNCH(1, false);
    }
#undef MEDT_AUG_LAUNCH
    return launch_status("augment_warp");
}

// --------------------------------------------------------------------------- //
// Exact squared Euclidean distance transform of uint8 masks (N,H,W) -> int32 (N,H,W), for the surface-distance scores
// (metrics.surface_scores: Hausdorff distance, its 95th percentile, average symmetric surface distance; not in the reference).
//   d2[y,x] = min over the feature pixels (y',x') of (y-y')^2 + (x-x')^2      MEDT_EDT_NONE where the image has none
// Feature set: mask != 0, or (border mode) the BORDER of mask != 0 -- the foreground pixels with a 4-neighbour outside the
// foreground, pixels outside the image counting as outside (MedPy's surface, A & ~binary_erosion(A, cross)).  Separable:
//   column pass  g2[y,x] = (distance along the column x to its nearest feature pixel)^2, or MEDT_EDT_NONE
//   row pass     d2[y,x] = min over x' of (x-x')^2 + g2[y,x']
// All integers (g <= 4095, so every sum stays below 2^26): the result is exact, and with no atomics the same on every run.
// The sentinel never enters a sum: the column pass tests for it before counting on, the row pass stages EDT_FAR in its place.
// --------------------------------------------------------------------------- //
constexpr int EDT_FAR = 1 << 30;              // what the row pass holds in LDS for MEDT_EDT_NONE: EDT_FAR + 4095^2 < 2^31
constexpr int EDT_ROWS = 8;                   // rows of a column whose loads the column pass issues together

struct alignas(16) EdtQuad {
    int32_t v[4];
};

// bit e: column e of the work-item's CPT columns is foreground.  (Flags are kept as bits of one word per row: arrays of
// bool would each live in a pair of scalar registers as a lane mask.)
template <int CPT>
__device__ __forceinline__ uint32_t edt_load_set(const uint8_t* __restrict__ p) {
    if (CPT == 4) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(p);
        uint32_t f = 0;
#pragma unroll
        for (int e = 0; e < CPT; ++e) f |= ((w >> (8 * e)) & 255u) ? 1u << e : 0u;
        return f;
    }
    return p[0] ? 1u : 0u;
}
template <int CPT>
__device__ __forceinline__ void edt_load_dist(const int32_t* __restrict__ p, int (&a)[CPT]) {
    if (CPT == 4) {
        const EdtQuad q = *reinterpret_cast<const EdtQuad*>(p);
#pragma unroll
        for (int e = 0; e < CPT; ++e) a[e] = q.v[e];
    } else {
        a[0] = p[0];
    }
}
template <int CPT>
__device__ __forceinline__ void edt_store_dist(int32_t* __restrict__ p, const int (&a)[CPT]) {
    if (CPT == 4) {
        EdtQuad q;
#pragma unroll
        for (int e = 0; e < CPT; ++e) q.v[e] = a[e];
        *reinterpret_cast<EdtQuad*>(p) = q;
    } else {
        p[0] = a[0];
    }
}

// A work-item owns CPT neighbouring columns of one image (4 with 16-byte stores, else 1), so neighbouring lanes touch
// neighbouring x.  Sweep down: the distance to the nearest feature pixel at or above, written to g2; sweep up: the one
// below, the smaller of the two squared.  The sweeps are serial in y, so each issues the loads of EDT_ROWS rows in front of
// the arithmetic.  Border mode derives the feature set from the mask as it goes (the rows y-1, y, y+1 of the own columns
// and one byte to either side); the border is never stored.
template <int CPT, bool BORDER>
__global__ __launch_bounds__(MEDT_THREADS) void edt_cols_kernel(const uint8_t* __restrict__ mask, int32_t* __restrict__ g2,
                                                                int H, int W, int bpi) {
    const int n = blockIdx.x / bpi;
    const int x0 = ((blockIdx.x - n * bpi) * blockDim.x + threadIdx.x) * CPT;
    if (x0 >= W) return;
    const uint8_t* m = mask + (size_t)n * H * W + x0;
    int32_t* g = g2 + (size_t)n * H * W + x0;
    constexpr uint32_t OWN = (1u << CPT) - 1u;
    int dist[CPT];
    uint32_t up = 0;                            // BORDER: the own columns of the row above the chunk (outside the image: 0)
#pragma unroll
    for (int e = 0; e < CPT; ++e) dist[e] = MEDT_EDT_NONE;
    for (int yb = 0; yb < H; yb += EDT_ROWS) {
        uint32_t c[EDT_ROWS + 1], side[EDT_ROWS];      // side: bit 0 the pixel left of the own columns, bit 1 the one right of them
#pragma unroll
        for (int r = 0; r <= EDT_ROWS; ++r) {
            const int y = yb + r;
            c[r] = 0;
            if (r < EDT_ROWS) side[r] = 0;
            if (y < H && (BORDER || r < EDT_ROWS)) {
                const uint8_t* row = m + (size_t)y * W;
                c[r] = edt_load_set<CPT>(row);
                if (BORDER && r < EDT_ROWS) {
                    if (x0 > 0 && row[-1] != 0) side[r] |= 1u;
                    if (x0 + CPT < W && row[CPT] != 0) side[r] |= 2u;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < EDT_ROWS; ++r) {
            const int y = yb + r;
            if (y >= H) break;
            uint32_t feat = c[r];
            if (BORDER) {
                const uint32_t above = r ? c[r ? r - 1 : 0] : up;
                const uint32_t left = ((c[r] << 1) | (side[r] & 1u)) & OWN, right = (c[r] >> 1) | ((side[r] >> 1) << (CPT - 1));
                feat &= ~(above & c[r + 1] & left & right);
            }
#pragma unroll
            for (int e = 0; e < CPT; ++e)
                dist[e] = ((feat >> e) & 1u) ? 0 : (dist[e] == MEDT_EDT_NONE ? MEDT_EDT_NONE : dist[e] + 1);
            edt_store_dist<CPT>(g + (size_t)y * W, dist);
        }
        up = c[EDT_ROWS - 1];
    }
#pragma unroll
    for (int e = 0; e < CPT; ++e) dist[e] = MEDT_EDT_NONE;
    for (int yb = H - 1; yb >= 0; yb -= EDT_ROWS) {
        int a[EDT_ROWS][CPT];
#pragma unroll
        for (int r = 0; r < EDT_ROWS; ++r)
            if (yb - r >= 0) edt_load_dist<CPT>(g + (size_t)(yb - r) * W, a[r]);
#pragma unroll
        for (int r = 0; r < EDT_ROWS; ++r) {
            const int y = yb - r;
            if (y < 0) break;
#pragma unroll
            for (int e = 0; e < CPT; ++e) {
                dist[e] = a[r][e] == 0 ? 0 : (dist[e] == MEDT_EDT_NONE ? MEDT_EDT_NONE : dist[e] + 1);
                const int d = min(a[r][e], dist[e]);
                a[r][e] = d == MEDT_EDT_NONE ? MEDT_EDT_NONE : d * d;
            }
            edt_store_dist<CPT>(g + (size_t)y * W, a[r]);
        }
    }
}

static inline unsigned edt_threads(int items) { return (unsigned)min(max((items + 63) / 64 * 64, 64), MEDT_THREADS); }

int edt_cols(const uint8_t* mask, int32_t* g2, int N, int H, int W, int border_mode, hipStream_t s) {
    const bool vec = (W % 4 == 0) && ((uintptr_t)mask % 4 == 0) && ((uintptr_t)g2 % 16 == 0);
    const int items = vec ? W / 4 : W;
    const unsigned threads = edt_threads(items);
    const int bpi = cdiv(items, (int)threads);
#define MEDT_EDT_COLS(CPT, BB) \
    hipLaunchKernelGGL((edt_cols_kernel<CPT, BB>), dim3((unsigned)N * bpi), dim3(threads), 0, s, mask, g2, H, W, bpi)
    if (vec) {
        if (border_mode) MEDT_EDT_COLS(4, true); else MEDT_EDT_COLS(4, false);
    } else {
        if (border_mode) MEDT_EDT_COLS(1, true); else MEDT_EDT_COLS(1, false);
    }
#undef MEDT_EDT_COLS
    return launch_status("edt_cols");
}

// One workgroup per (image, row): the row of g2 in LDS; a work-item owns the pixels x = tid, tid + threads, ... (neighbouring
// lanes read neighbouring LDS words at every step of the search) and walks outwards from x, both sides at once, until
// (x-x')^2 alone reaches the best value so far.  SELECT: only the border pixels of `select` are searched, the others
// receive -1.  VEC4: 16-byte loads of g2, and the results go through LDS to leave as 16-byte stores.
template <bool VEC4, bool SELECT>
__global__ __launch_bounds__(MEDT_THREADS) void edt_rows_kernel(const int32_t* __restrict__ g2,
                                                                const uint8_t* __restrict__ select, int32_t* __restrict__ d2,
                                                                int H, int W) {
    MEDT_STATIC_SHARED EdtQuad gq[MEDT_EDT_MAX_DIM / 4], oq[MEDT_EDT_MAX_DIM / 4];
    int32_t* gs = reinterpret_cast<int32_t*>(gq);
    int32_t* os = reinterpret_cast<int32_t*>(oq);
    const int n = blockIdx.x / H, y = blockIdx.x - n * H, tid = threadIdx.x, T = blockDim.x;
    const size_t row = ((size_t)n * H + y) * W;
    if (VEC4) {
        for (int i = tid; i < W / 4; i += T) {
            EdtQuad q = reinterpret_cast<const EdtQuad*>(g2 + row)[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) q.v[e] = min(q.v[e], EDT_FAR);
            gq[i] = q;
        }
    } else {
        for (int x = tid; x < W; x += T) gs[x] = min(g2[row + x], EDT_FAR);
    }
    __syncthreads();
    for (int x = tid; x < W; x += T) {
        bool wanted = true;
        if (SELECT) {
            const uint8_t* c = select + row + x;
            wanted = c[0] != 0 && (x == 0 || x == W - 1 || y == 0 || y == H - 1 || c[-1] == 0 || c[1] == 0 || c[-W] == 0 || c[W] == 0);
        }
        int best = -1;
        if (wanted) {
            best = gs[x];
            const int reach = max(x, W - 1 - x);
            for (int d = 1; d <= reach; ++d) {
                const int dd = d * d;
                if (dd >= best) break;
                if (x - d >= 0) best = min(best, gs[x - d] + dd);
                if (x + d < W) best = min(best, gs[x + d] + dd);
            }
            if (best >= EDT_FAR) best = MEDT_EDT_NONE;
        }
        if (VEC4) os[x] = best; else d2[row + x] = best;
    }
    if (VEC4) {
        __syncthreads();
        for (int i = tid; i < W / 4; i += T) reinterpret_cast<EdtQuad*>(d2 + row)[i] = oq[i];
    }
}

int edt_rows(const int32_t* g2, const uint8_t* select, int32_t* d2, int N, int H, int W, hipStream_t s) {
    const bool vec = (W % 4 == 0) && ((uintptr_t)g2 % 16 == 0) && ((uintptr_t)d2 % 16 == 0);
    const dim3 grid((unsigned)N * H), block(edt_threads(W));
#define MEDT_EDT_ROWS(VV, SS) hipLaunchKernelGGL((edt_rows_kernel<VV, SS>), grid, block, 0, s, g2, select, d2, H, W)
    if (vec) {
        if (select) MEDT_EDT_ROWS(true, true); else MEDT_EDT_ROWS(true, false);
    } else {
        if (select) MEDT_EDT_ROWS(false, true); else MEDT_EDT_ROWS(false, false);
    }
#undef MEDT_EDT_ROWS
    return launch_status("edt_rows");
}

// --------------------------------------------------------------------------- //
// Signed squared distance map of a label map, for the boundary loss of the training step (Kervadec et al., MIDL 2019):
//   F = {target == fg};  sd2 = +d^2 to the nearest pixel of F outside F, -d^2 to the nearest pixel outside F inside it,
//   0 everywhere in an image that has no F pixel or no other pixel.
// The training-path sibling of the transform above: class indices in, small maps (4 x 128^2 in a step), two launches.
// Column pass: the distance along the column to the nearest F pixel is wanted at the pixels outside F and is 0 inside; the
// distance to the nearest pixel outside F is wanted inside F and is 0 outside.  The two maps never both hold a value at one
// pixel, so they share one int32 word: g2 > 0 outside F (the first map), g2 < 0 inside (minus the second), +-EDT_FAR where the
// column has no pixel of the other set.  The row pass reads the query pixel's own set from the sign of its own word and takes
// max(+-g2, 0) as the column term of the others.
// A column is cut into words of 32 rows; a work-item owns one word of one column, EDT_SCOLS neighbouring columns side by side
// in the lanes.  Its 32 loads are independent; the set bits go to LDS, where a word finds the nearest pixel of either set
// above and below it in the other words of its column; inside the word the neighbours come from bit scans.  No sweep carries a
// dependency through global memory, and 128 rows are 4 work-items deep instead of 2 x 128 dependent steps.
// --------------------------------------------------------------------------- //
constexpr int EDT_SCOLS = 16;                                // columns per workgroup of the signed column pass
constexpr int EDT_SWORDS = MEDT_EDT_MAX_DIM / 32;            // 32-row words per column at most
constexpr int EDT_SOFF = 1 << 15;                            // a row further off than any pixel: (EDT_SOFF)^2 = EDT_FAR

// squared distance from row y to the nearest set bit of `other` (bits of the rows y0 .. y0+31), or to `up` / `dn`, the
// nearest such rows outside the word (-EDT_SOFF / 2 * EDT_SOFF when there is none); EDT_FAR when the column has none
__device__ __forceinline__ int edt_signed_col_d2(uint32_t other, int r, int y0, int up, int dn) {
    const uint32_t below = other & ((1u << r) - 1u), above = (other >> r) >> 1;
    const int y = y0 + r;
    const int a = below ? y0 + 31 - __builtin_clz(below) : up;
    const int b = above ? y + 1 + __builtin_ctz(above) : dn;
    const int d = min(y - a, b - y);
    return d >= EDT_SOFF ? EDT_FAR : d * d;
}

__global__ __launch_bounds__(MEDT_THREADS) void signed_edt_cols_kernel(const int64_t* __restrict__ target,
                                                                       int32_t* __restrict__ g2, int H, int W, int tiles,
                                                                       int words, int fg, int ignore) {
    MEDT_STATIC_SHARED uint32_t bits[EDT_SWORDS * EDT_SCOLS];
    const int n = blockIdx.x / tiles;
    const int c = threadIdx.x % EDT_SCOLS, slot = threadIdx.x / EDT_SCOLS, slots = blockDim.x / EDT_SCOLS;
    const int x = (blockIdx.x - n * tiles) * EDT_SCOLS + c;
    const int64_t* t = target + (size_t)n * H * W + x;
    int32_t* g = g2 + (size_t)n * H * W + x;
    if (x < W) {
        for (int w = slot; w < words; w += slots) {
            const int y0 = w * 32, rows = min(32, H - y0);
            uint32_t f = 0;
#pragma unroll 8
            for (int r = 0; r < rows; ++r) {
                const int64_t v = t[(size_t)(y0 + r) * W];
                f |= (v == fg && v != ignore) ? 1u << r : 0u;
            }
            bits[w * EDT_SCOLS + c] = f;
        }
    }
    __syncthreads();
    if (x >= W) return;
    for (int w = slot; w < words; w += slots) {
        const int y0 = w * 32, rows = min(32, H - y0);
        const uint32_t valid = rows == 32 ? 0xffffffffu : (1u << rows) - 1u;
        const uint32_t f = bits[w * EDT_SCOLS + c], o = ~f & valid;
        int upF = -EDT_SOFF, upO = -EDT_SOFF, dnF = 2 * EDT_SOFF, dnO = 2 * EDT_SOFF;
        for (int v = w - 1; v >= 0 && (upF < 0 || upO < 0); --v) {          // every word above the last is full
            const uint32_t m = bits[v * EDT_SCOLS + c], mo = ~m;
            if (upF < 0 && m) upF = v * 32 + 31 - __builtin_clz(m);
            if (upO < 0 && mo) upO = v * 32 + 31 - __builtin_clz(mo);
        }
        for (int v = w + 1; v < words && (dnF >= EDT_SOFF || dnO >= EDT_SOFF); ++v) {
            const int vr = min(32, H - v * 32);
            const uint32_t m = bits[v * EDT_SCOLS + c], mo = ~m & (vr == 32 ? 0xffffffffu : (1u << vr) - 1u);
            if (dnF >= EDT_SOFF && m) dnF = v * 32 + __builtin_ctz(m);
            if (dnO >= EDT_SOFF && mo) dnO = v * 32 + __builtin_ctz(mo);
        }
#pragma unroll 8
        for (int r = 0; r < rows; ++r) {
            const bool in = (f >> r) & 1u;
            const int d2 = in ? edt_signed_col_d2(o, r, y0, upO, dnO) : edt_signed_col_d2(f, r, y0, upF, dnF);
            g[(size_t)(y0 + r) * W] = in ? -d2 : d2;
        }
    }
}

// Rows of the signed column map in LDS, 256 / T of them per workgroup when a row needs only T < 256 work-items (rpb; two at
// 128 columns).  The search of edt_rows_kernel with the column term taken from the side of the query pixel's own sign.
__global__ __launch_bounds__(MEDT_THREADS) void signed_edt_rows_kernel(const int32_t* __restrict__ g2, int32_t* __restrict__ sd2,
                                                                       int W, int T, int rpb, int nrows) {
    MEDT_STATIC_SHARED int32_t gs[MEDT_EDT_MAX_DIM];
    const int rr = threadIdx.x / T, lx = threadIdx.x - rr * T;
    const int rowi = blockIdx.x * rpb + rr;
    const bool live = rr < rpb && rowi < nrows;
    const size_t row = (size_t)(live ? rowi : 0) * W;
    int32_t* my = gs + rr * T;                                  // rpb > 1 only when W <= T
    if (live)
        for (int x = lx; x < W; x += T) my[x] = g2[row + x];
    __syncthreads();
    if (!live) return;
    for (int x = lx; x < W; x += T) {
        const int own = my[x], s = own < 0 ? -1 : 1;
        int best = own * s;                                   // the own column: the distance to the other set along it
        const int reach = max(x, W - 1 - x);
        for (int d = 1; d <= reach; ++d) {
            const int dd = d * d;
            if (dd >= best) break;
            if (x - d >= 0) best = min(best, max(my[x - d] * s, 0) + dd);
            if (x + d < W) best = min(best, max(my[x + d] * s, 0) + dd);
        }
        sd2[row + x] = best >= EDT_FAR ? 0 : best * s;
    }
}

int signed_edt(const int64_t* target, int32_t* g2, int32_t* sd2, int N, int H, int W, int fg, int ignore, hipStream_t s) {
    const int words = cdiv(H, 32), tiles = cdiv(W, EDT_SCOLS);
    const unsigned cthreads = (unsigned)min(max(cdiv(words * EDT_SCOLS, 64) * 64, 64), MEDT_THREADS);
    hipLaunchKernelGGL(signed_edt_cols_kernel, dim3((unsigned)N * tiles), dim3(cthreads), 0, s, target, g2, H, W, tiles, words,
                       fg, ignore);
    if (int rc = launch_status("signed_edt_cols")) return rc;
    const int T = (int)edt_threads(W), rpb = W <= T ? MEDT_THREADS / T : 1, nrows = N * H;
    hipLaunchKernelGGL(signed_edt_rows_kernel, dim3((unsigned)cdiv(nrows, rpb)), dim3((unsigned)(T * rpb)), 0, s, g2, sd2, W, T,
                       rpb, nrows);
    return launch_status("signed_edt_rows");
}

// --------------------------------------------------------------------------- //
// Boundary term of the loss:  B = mean over images n of ( sum over valid p of phi_n(p) s_n(p) / max(1, V_n) ),
//   s = softmax(logits)[fg],  phi = sqrt(sd2) outside F, -(sqrt(-sd2) - 1) inside (0 on the inner border), 0 where sd2 == 0
//   (Kervadec's one_hot2dist), computed from the integers on the fly; valid: target in [0, K) and not `ignore`; V_n their count.
// The grid of the segmentation loss above: a workgroup never straddles two images.  partials [N][bpi][2] = {sum phi s, V};
// the finalize sums them in double in a fixed order and reads the weight alpha from device memory:
//   out = [base + alpha B (alpha B when base is NULL), B, alpha, 1 / (N max(1, V_n)) for n < N]
// The backward reads alpha and the last N floats again; with `accumulate` it adds into the dlogits the region loss's backward
// wrote (one buffer, no second gradient tensor), else it writes, zeros at the pixels that are not valid included.
// --------------------------------------------------------------------------- //
__device__ __forceinline__ float boundary_phi(int sd2) {
    if (sd2 > 0) return sqrtf((float)sd2);
    if (sd2 < 0) return 1.f - sqrtf((float)-sd2);
    return 0.f;
}

__global__ __launch_bounds__(MEDT_THREADS) void boundary_fwd_kernel(const float* __restrict__ logits,
                                                                    const int64_t* __restrict__ target,
                                                                    const int32_t* __restrict__ sd2,
                                                                    float* __restrict__ partials, int K, int HW, int bpi,
                                                                    int fg, int ignore) {
    MEDT_STATIC_SHARED float red[MEDT_WAVES * 2];
    const int n = blockIdx.x / bpi;
    const int p = (blockIdx.x - n * bpi) * MEDT_THREADS + threadIdx.x;
    float v[2] = {0.f, 0.f};
    if (p < HW) {
        const int64_t t = target[(size_t)n * HW + p];
        if (t != ignore && t >= 0 && t < K) {
            const float* lp = logits + (size_t)n * K * HW + p;
            float m = lp[0];
            for (int k = 1; k < K; ++k) m = fmaxf(m, lp[(size_t)k * HW]);
            float sum = 0.f;
            for (int k = 0; k < K; ++k) sum += __expf(lp[(size_t)k * HW] - m);
            v[0] = boundary_phi(sd2[(size_t)n * HW + p]) * (__expf(lp[(size_t)fg * HW] - m) / sum);
            v[1] = 1.f;
        }
    }
    block_sum<2>(v, red, partials + (size_t)blockIdx.x * 2);
}

// One workgroup; wave w sums the partial rows of the images w, w + 4, .. in double, thread 0 adds the waves' totals in order.
__global__ __launch_bounds__(MEDT_THREADS) void boundary_finalize_kernel(const float* __restrict__ partials,
                                                                         const float* __restrict__ alpha,
                                                                         const float* __restrict__ base,
                                                                         float* __restrict__ out, int N, int bpi) {
    MEDT_STATIC_SHARED double tot[MEDT_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double sb = 0.0;
    for (int n = wave; n < N; n += MEDT_WAVES) {
        double a = 0.0, c = 0.0;
        for (int b = lane; b < bpi; b += 64) {
            const float* pp = partials + ((size_t)n * bpi + b) * 2;
            a += (double)pp[0];
            c += (double)pp[1];
        }
        a = wave_sum_d(a);
        c = wave_sum_d(c);
        const double cnt = c > 1.0 ? c : 1.0;
        sb += a / cnt;
        if (lane == 0) out[3 + n] = (float)(1.0 / (cnt * (double)N));
    }
    if (lane == 0) tot[wave] = sb;
    __syncthreads();
    if (threadIdx.x == 0) {
        double B = 0.0;
        for (int w = 0; w < MEDT_WAVES; ++w) B += tot[w];
        B /= (double)N;
        const float al = alpha[0];
        const double term = (double)al * B;
        out[0] = (float)(base ? (double)base[0] + term : term);
        out[1] = (float)B;
        out[2] = al;
    }
}

// dlogits[n,k,p] (+)= dloss alpha phi / (N max(1, V_n)) * s (delta_k,fg - p_k)
template <bool ACC>
__global__ __launch_bounds__(MEDT_THREADS) void boundary_bwd_kernel(const float* __restrict__ logits,
                                                                    const int64_t* __restrict__ target,
                                                                    const int32_t* __restrict__ sd2,
                                                                    const float* __restrict__ out,
                                                                    const float* __restrict__ dloss,
                                                                    float* __restrict__ dlogits, int K, int HW, int bpi, int fg,
                                                                    int ignore) {
    const int n = blockIdx.x / bpi;
    const int p = (blockIdx.x - n * bpi) * MEDT_THREADS + threadIdx.x;
    if (p >= HW) return;
    const int64_t t = target[(size_t)n * HW + p];
    const float* lp = logits + (size_t)n * K * HW + p;
    float* dp = dlogits + (size_t)n * K * HW + p;
    if (t == ignore || t < 0 || t >= K) {
        if (!ACC)
            for (int k = 0; k < K; ++k) dp[(size_t)k * HW] = 0.f;
        return;                                               // ACC: the region loss's backward wrote the zeros
    }
    float m = lp[0];
    for (int k = 1; k < K; ++k) m = fmaxf(m, lp[(size_t)k * HW]);
    float sum = 0.f;
    for (int k = 0; k < K; ++k) sum += __expf(lp[(size_t)k * HW] - m);
    const float inv = 1.f / sum;
    const float sf = __expf(lp[(size_t)fg * HW] - m) * inv;
    const float c = (dloss ? dloss[0] : 1.f) * out[2] * out[3 + n] * boundary_phi(sd2[(size_t)n * HW + p]) * sf;
    for (int k = 0; k < K; ++k) {
        const float pk = __expf(lp[(size_t)k * HW] - m) * inv;
        const float gk = c * ((k == fg ? 1.f : 0.f) - pk);
        dp[(size_t)k * HW] = ACC ? dp[(size_t)k * HW] + gk : gk;
    }
}

size_t boundary_partials(int N, int HW) { return (size_t)N * seg_loss_bpi(HW) * 2; }
size_t boundary_out_floats(int N) { return 3 + (size_t)N; }

int boundary_fwd(const float* logits, const int64_t* target, const int32_t* sd2, const float* alpha, const float* base,
                 float* partials, float* out, int N, int K, int HW, int fg, int ignore, hipStream_t s) {
    const int bpi = seg_loss_bpi(HW);
    hipLaunchKernelGGL(boundary_fwd_kernel, dim3((unsigned)N * bpi), dim3(MEDT_THREADS), 0, s, logits, target, sd2, partials, K,
                       HW, bpi, fg, ignore);
    if (int rc = launch_status("boundary_fwd")) return rc;
    hipLaunchKernelGGL(boundary_finalize_kernel, dim3(1), dim3(MEDT_THREADS), 0, s, partials, alpha, base, out, N, bpi);
    return launch_status("boundary_finalize");
}

int boundary_bwd(const float* logits, const int64_t* target, const int32_t* sd2, const float* out, const float* dloss,
                 float* dlogits, int N, int K, int HW, int fg, int ignore, int accumulate, hipStream_t s) {
    const int bpi = seg_loss_bpi(HW);
    const dim3 grid((unsigned)N * bpi), block(MEDT_THREADS);
    if (accumulate)
        hipLaunchKernelGGL(boundary_bwd_kernel<true>, grid, block, 0, s, logits, target, sd2, out, dloss, dlogits, K, HW, bpi, fg,
                           ignore);
    else
        hipLaunchKernelGGL(boundary_bwd_kernel<false>, grid, block, 0, s, logits, target, sd2, out, dloss, dlogits, K, HW, bpi,
                           fg, ignore);
    return launch_status("boundary_bwd");
}

// --------------------------------------------------------------------------- //
// Two-nearest-object distance transform of a label map (0 = no object, l > 0 = object l; label.hip writes such maps), for the
// border weight of the training step (Ronneberger et al., U-Net, 2015):
//   d1sq = squared distance to the nearest labelled pixel, d2sq = squared distance to the nearest labelled pixel of ANOTHER
//   object than the one that attains d1sq -- the two smallest of the per-object minimum distances; MEDT_EDT_NONE where the image
//   has no such object.  Labels are not returned: under ties they are not unique, the two distances are.
// Column pass: per pixel the nearest labelled pixel of its column, (g1, a), and the nearest one whose label is not a, (g2, b):
// four planes of N*H*W int32 in `scratch`, g1 | a | g2 | b, EDT_FAR and label 0 where the column has none.
// The shape of signed_edt_cols_kernel, with segments for its 32-row words: a work-item owns EDT2_SEG rows of one column, 16
// neighbouring columns side by side in the lanes (8 above 2048 rows, so that the summaries fit 48 KB of LDS).  Its loads are
// independent.  A sweep along a column carries the two-deep state (y_a, a), (y_b, b): a labelled pixel of label a moves y_a, any
// other label pushes (y_a, a) into second place -- so y_b is always the last row whose label was not a.  A segment puts into LDS
// what such a sweep would see of it from above and from below (its first labelled row and the first row of another label, from
// either end); after the barrier a work-item builds the state entering its segment from the summaries above it, nearest first,
// until both places are filled (edt2_offer_segment), sweeps its rows downward into registers, does the same from below and
// merges the two pairs with edt2_take on the way up.  No sweep carries a dependency through global memory.
// Row pass: the search of signed_edt_rows_kernel, fed both entries of every column, keeping the best pair of distinct labels.
// Two entries per column suffice: if the second-nearest object reaches the pixel through a column where it is third or further
// along the column, two other labels of that column are at least as close, one of them is not the nearest object's, and it
// gives a distance no larger.
// --------------------------------------------------------------------------- //
constexpr int EDT2_SEG = 16;                                 // rows of a column a work-item owns
constexpr int EDT2_ENTRIES = 2048;                           // (segment, column) pairs of a workgroup: 16 columns up to 2048 rows, 8 beyond

// (b1, l1), (b2, l2): the two nearest so far, of distinct labels (label 0: none yet).  Offers (v, l); l == 0 is no candidate.
__device__ __forceinline__ void edt2_take(int v, int l, int& b1, int& l1, int& b2, int& l2) {
    if (l == 0) return;
    if (l == l1) b1 = min(b1, v);
    else if (v < b1) { b2 = b1; l2 = l1; b1 = v; l1 = l; }
    else if (l == l2) b2 = min(b2, v);
    else if (v < b2) { b2 = v; l2 = l; }
}

// One step of a sweep along a column: the state (ya, a), (yb, b) -- the last labelled row and its label, the last row whose label
// was not a -- meets label l at row y.
__device__ __forceinline__ void edt2_step(int y, int l, int& ya, int& a, int& yb, int& b) {
    if (l > 0) {
        if (l != a) { yb = ya; b = a; a = l; }
        ya = y;
    }
}

// A state that still lacks a or b is offered the labelled row r of label l (l <= 0: none); nearer rows were offered first.
__device__ __forceinline__ void edt2_offer(int r, int l, int& ya, int& a, int& yb, int& b) {
    const bool first = l > 0 && a == 0, second = l > 0 && a != 0 && b == 0 && l != a;     // (selects: the state stays in registers)
    ya = first ? r : ya;
    a = first ? l : a;
    yb = second ? r : yb;
    b = second ? l : b;
}

// ... a segment's summary as seen from outside: {rows r1 | r2 << 16, l1, l2}, (r1, l1) its labelled row nearest to the viewer and
// (r2, l2) the nearest one whose label is not l1.
__device__ __forceinline__ void edt2_offer_segment(int rows, int l1, int l2, int& ya, int& a, int& yb, int& b) {
    edt2_offer(rows & 0xffff, l1, ya, a, yb, b);
    edt2_offer(rows >> 16, l2, ya, a, yb, b);
}

__global__ __launch_bounds__(MEDT_THREADS) void object_edt2_cols_kernel(const int32_t* __restrict__ labels,
                                                                        int32_t* __restrict__ scratch, int H, int W, int tiles,
                                                                        int segs, int cpw, size_t plane) {
    // per (segment, column): from the top {rows r1 | r2 << 16, l1, l2}, from the bottom the same
    MEDT_STATIC_SHARED int32_t sum[6 * EDT2_ENTRIES];
    const int n = blockIdx.x / tiles;
    const int c = threadIdx.x % cpw, slot = threadIdx.x / cpw, slots = blockDim.x / cpw;
    const int x = (blockIdx.x - n * tiles) * cpw + c;
    const int32_t* lab = labels + (size_t)n * H * W + x;
    if (x < W) {
        for (int w = slot; w < segs; w += slots) {
            const int y0 = w * EDT2_SEG;
            int l[EDT2_SEG];
#pragma unroll
            for (int k = 0; k < EDT2_SEG; ++k) l[k] = y0 + k < H ? lab[(size_t)(y0 + k) * W] : 0;
            int ya = 0, a = 0, yb = 0, b = 0;                  // from the top: the FIRST labelled row, the first of another label
#pragma unroll
            for (int k = 0; k < EDT2_SEG; ++k) edt2_offer(y0 + k, l[k], ya, a, yb, b);
            int* e = sum + w * cpw + c;
            e[0] = ya | (yb << 16);
            e[EDT2_ENTRIES] = a;
            e[2 * EDT2_ENTRIES] = b;
            ya = a = yb = b = 0;                               // from the bottom
#pragma unroll
            for (int k = EDT2_SEG - 1; k >= 0; --k) edt2_offer(y0 + k, l[k], ya, a, yb, b);
            e[3 * EDT2_ENTRIES] = ya | (yb << 16);
            e[4 * EDT2_ENTRIES] = a;
            e[5 * EDT2_ENTRIES] = b;
        }
    }
    __syncthreads();
    if (x >= W) return;
    int32_t* G1 = scratch + (size_t)n * H * W + x;
    int32_t *A = G1 + plane, *G2 = A + plane, *B = G2 + plane;
    for (int w = slot; w < segs; w += slots) {
        const int y0 = w * EDT2_SEG;
        int l[EDT2_SEG], dn[EDT2_SEG], da[EDT2_SEG], db[EDT2_SEG];
#pragma unroll
        for (int k = 0; k < EDT2_SEG; ++k) l[k] = y0 + k < H ? lab[(size_t)(y0 + k) * W] : 0;
        int ya = 0, a = 0, yb = 0, b = 0;                      // what the segments above hold, nearest first
        for (int v = w - 1; v >= 0 && b == 0; --v) {
            const int* e = sum + v * cpw + c;
            edt2_offer_segment(e[3 * EDT2_ENTRIES], e[4 * EDT2_ENTRIES], e[5 * EDT2_ENTRIES], ya, a, yb, b);
        }
#pragma unroll
        for (int k = 0; k < EDT2_SEG; ++k) {                   // downward: vertical distances (< 4096 each) and labels, in registers
            const int y = y0 + k;
            edt2_step(y, l[k], ya, a, yb, b);
            dn[k] = (y - ya) | ((y - yb) << 16);
            da[k] = a;
            db[k] = b;
        }
        ya = a = yb = b = 0;                                   // what the segments below hold
        for (int v = w + 1; v < segs && b == 0; ++v) {
            const int* e = sum + v * cpw + c;
            edt2_offer_segment(e[0], e[EDT2_ENTRIES], e[2 * EDT2_ENTRIES], ya, a, yb, b);
        }
#pragma unroll
        for (int k = EDT2_SEG - 1; k >= 0; --k) {              // upward, merged with the downward pair
            const int y = y0 + k;
            if (y >= H) continue;
            edt2_step(y, l[k], ya, a, yb, b);
            const int d1 = dn[k] & 0xffff, d2 = dn[k] >> 16;
            int b1 = da[k] ? d1 * d1 : EDT_FAR, l1 = da[k], b2 = db[k] ? d2 * d2 : EDT_FAR, l2 = db[k];
            edt2_take((ya - y) * (ya - y), a, b1, l1, b2, l2);
            edt2_take((yb - y) * (yb - y), b, b1, l1, b2, l2);
            const size_t o = (size_t)y * W;
            G1[o] = b1;
            A[o] = l1;
            G2[o] = b2;
            B[o] = l2;
        }
    }
}

// Rows of the four planes in LDS, 256 / T rows per workgroup when a row needs only T < 256 work-items (as the signed row pass).
__global__ __launch_bounds__(MEDT_THREADS) void object_edt2_rows_kernel(const int32_t* __restrict__ scratch,
                                                                        int32_t* __restrict__ d1sq, int32_t* __restrict__ d2sq,
                                                                        int W, int T, int rpb, int nrows, size_t plane) {
    MEDT_STATIC_SHARED int32_t s1[MEDT_EDT_MAX_DIM], sa[MEDT_EDT_MAX_DIM], s2[MEDT_EDT_MAX_DIM], sb[MEDT_EDT_MAX_DIM];
    const int rr = threadIdx.x / T, lx = threadIdx.x - rr * T;
    const int rowi = blockIdx.x * rpb + rr;
    const bool live = rr < rpb && rowi < nrows;
    const size_t row = (size_t)(live ? rowi : 0) * W;
    const int base = rr * T;                                    // rpb > 1 only when W <= T
    if (live)
        for (int x = lx; x < W; x += T) {
            s1[base + x] = scratch[row + x];
            sa[base + x] = scratch[plane + row + x];
            s2[base + x] = scratch[2 * plane + row + x];
            sb[base + x] = scratch[3 * plane + row + x];
        }
    __syncthreads();
    if (!live) return;
    for (int x = lx; x < W; x += T) {
        int b1 = EDT_FAR, l1 = 0, b2 = EDT_FAR, l2 = 0;
        edt2_take(s1[base + x], sa[base + x], b1, l1, b2, l2);
        edt2_take(s2[base + x], sb[base + x], b1, l1, b2, l2);
        const int reach = max(x, W - 1 - x);
        for (int d = 1; d <= reach; ++d) {
            const int dd = d * d;
            if (dd >= b2) break;
            if (x - d >= 0) {
                const int i = base + x - d;
                edt2_take(s1[i] + dd, sa[i], b1, l1, b2, l2);
                edt2_take(s2[i] + dd, sb[i], b1, l1, b2, l2);
            }
            if (x + d < W) {
                const int i = base + x + d;
                edt2_take(s1[i] + dd, sa[i], b1, l1, b2, l2);
                edt2_take(s2[i] + dd, sb[i], b1, l1, b2, l2);
            }
        }
        d1sq[row + x] = b1 >= EDT_FAR ? MEDT_EDT_NONE : b1;
        d2sq[row + x] = b2 >= EDT_FAR ? MEDT_EDT_NONE : b2;
    }
}

int object_edt2(const int32_t* labels, int32_t* scratch, int32_t* d1sq, int32_t* d2sq, int N, int H, int W, hipStream_t s) {
    const int segs = cdiv(H, EDT2_SEG), cpw = segs * 16 <= EDT2_ENTRIES ? 16 : 8, tiles = cdiv(W, cpw);
    const size_t plane = (size_t)N * H * W;
    const unsigned cthreads = (unsigned)min(max(cdiv(segs * cpw, 64) * 64, 64), MEDT_THREADS);
    hipLaunchKernelGGL(object_edt2_cols_kernel, dim3((unsigned)N * tiles), dim3(cthreads), 0, s, labels, scratch, H, W, tiles, segs,
                       cpw, plane);
    if (int rc = launch_status("object_edt2_cols")) return rc;
    const int T = (int)edt_threads(W), rpb = W <= T ? MEDT_THREADS / T : 1, nrows = N * H;
    hipLaunchKernelGGL(object_edt2_rows_kernel, dim3((unsigned)cdiv(nrows, rpb)), dim3((unsigned)(T * rpb)), 0, s, scratch, d1sq,
                       d2sq, W, T, rpb, nrows, plane);
    return launch_status("object_edt2_rows");
}

// --------------------------------------------------------------------------- //
// Border term of the loss (U-Net's weight map for touching objects, as an additive term):
//   R = mean over images n of ( sum over valid p of e_n(p) nll_n(p) / max(1, V_n) ),  nll = -log softmax(logits)[target],
//   e = exp(-(sqrt(d1sq) + sqrt(d2sq))^2 / (2 sigma^2)) at the pixels outside F = {target == fg} whose d2sq is not
//   MEDT_EDT_NONE, 0 elsewhere; computed from the integers on the fly.  Valid pixels, V_n, the grid, the partials [N][bpi][2]
//   = {sum e nll, V} and `out` are the boundary term's, and so is the finalize (boundary_finalize_kernel, w0 for alpha):
//   out = [base + w0 R (w0 R when base is NULL), R, w0, 1 / (N max(1, V_n)) for n < N]
// --------------------------------------------------------------------------- //
__device__ __forceinline__ float border_e(int64_t t, int fg, int d1, int d2, float inv2s2) {
    if (t == fg || d2 == MEDT_EDT_NONE) return 0.f;
    const float s = sqrtf((float)d1) + sqrtf((float)d2);
    return __expf(-(s * s) * inv2s2);
}

__global__ __launch_bounds__(MEDT_THREADS) void border_fwd_kernel(const float* __restrict__ logits,
                                                                  const int64_t* __restrict__ target,
                                                                  const int32_t* __restrict__ d1sq,
                                                                  const int32_t* __restrict__ d2sq, float* __restrict__ partials,
                                                                  int K, int HW, int bpi, int fg, int ignore, float inv2s2) {
    MEDT_STATIC_SHARED float red[MEDT_WAVES * 2];
    const int n = blockIdx.x / bpi;
    const int p = (blockIdx.x - n * bpi) * MEDT_THREADS + threadIdx.x;
    float v[2] = {0.f, 0.f};
    if (p < HW) {
        const int64_t t = target[(size_t)n * HW + p];
        if (t != ignore && t >= 0 && t < K) {
            v[1] = 1.f;
            const float e = border_e(t, fg, d1sq[(size_t)n * HW + p], d2sq[(size_t)n * HW + p], inv2s2);
            if (e != 0.f) {
                const float* lp = logits + (size_t)n * K * HW + p;
                float m = lp[0];
                for (int k = 1; k < K; ++k) m = fmaxf(m, lp[(size_t)k * HW]);
                float sum = 0.f;
                for (int k = 0; k < K; ++k) sum += __expf(lp[(size_t)k * HW] - m);
                v[0] = e * (m + __logf(sum) - lp[(size_t)t * HW]);
            }
        }
    }
    block_sum<2>(v, red, partials + (size_t)blockIdx.x * 2);
}

// dlogits[n,k,p] (+)= dloss w0 e / (N max(1, V_n)) * (p_k - delta_k,t)
template <bool ACC>
__global__ __launch_bounds__(MEDT_THREADS) void border_bwd_kernel(const float* __restrict__ logits,
                                                                  const int64_t* __restrict__ target,
                                                                  const int32_t* __restrict__ d1sq,
                                                                  const int32_t* __restrict__ d2sq, const float* __restrict__ out,
                                                                  const float* __restrict__ dloss, float* __restrict__ dlogits,
                                                                  int K, int HW, int bpi, int fg, int ignore, float inv2s2) {
    const int n = blockIdx.x / bpi;
    const int p = (blockIdx.x - n * bpi) * MEDT_THREADS + threadIdx.x;
    if (p >= HW) return;
    const int64_t t = target[(size_t)n * HW + p];
    const float* lp = logits + (size_t)n * K * HW + p;
    float* dp = dlogits + (size_t)n * K * HW + p;
    const bool valid = t != ignore && t >= 0 && t < K;
    const float e = valid ? border_e(t, fg, d1sq[(size_t)n * HW + p], d2sq[(size_t)n * HW + p], inv2s2) : 0.f;
    if (e == 0.f) {                                           // not valid, inside F, or no second object: no gradient
        if (!ACC)
            for (int k = 0; k < K; ++k) dp[(size_t)k * HW] = 0.f;
        return;                                               // ACC: the region loss's backward wrote this pixel
    }
    float m = lp[0];
    for (int k = 1; k < K; ++k) m = fmaxf(m, lp[(size_t)k * HW]);
    float sum = 0.f;
    for (int k = 0; k < K; ++k) sum += __expf(lp[(size_t)k * HW] - m);
    const float inv = 1.f / sum;
    const float c = (dloss ? dloss[0] : 1.f) * out[2] * out[3 + n] * e;
    for (int k = 0; k < K; ++k) {
        const float pk = __expf(lp[(size_t)k * HW] - m) * inv;
        const float gk = c * (pk - (k == t ? 1.f : 0.f));
        dp[(size_t)k * HW] = ACC ? dp[(size_t)k * HW] + gk : gk;
    }
}

int border_fwd(const float* logits, const int64_t* target, const int32_t* d1sq, const int32_t* d2sq, float sigma, const float* w0,
               const float* base, float* partials, float* out, int N, int K, int HW, int fg, int ignore, hipStream_t s) {
    const int bpi = seg_loss_bpi(HW);
    const float inv2s2 = (float)(1.0 / (2.0 * (double)sigma * (double)sigma));
    hipLaunchKernelGGL(border_fwd_kernel, dim3((unsigned)N * bpi), dim3(MEDT_THREADS), 0, s, logits, target, d1sq, d2sq, partials,
                       K, HW, bpi, fg, ignore, inv2s2);
    if (int rc = launch_status("border_fwd")) return rc;
    hipLaunchKernelGGL(boundary_finalize_kernel, dim3(1), dim3(MEDT_THREADS), 0, s, partials, w0, base, out, N, bpi);
    return launch_status("border_finalize");
}

int border_bwd(const float* logits, const int64_t* target, const int32_t* d1sq, const int32_t* d2sq, float sigma, const float* out,
               const float* dloss, float* dlogits, int N, int K, int HW, int fg, int ignore, int accumulate, hipStream_t s) {
    const int bpi = seg_loss_bpi(HW);
    const float inv2s2 = (float)(1.0 / (2.0 * (double)sigma * (double)sigma));
    const dim3 grid((unsigned)N * bpi), block(MEDT_THREADS);
    if (accumulate)
        hipLaunchKernelGGL(border_bwd_kernel<true>, grid, block, 0, s, logits, target, d1sq, d2sq, out, dloss, dlogits, K, HW, bpi,
                           fg, ignore, inv2s2);
    else
        hipLaunchKernelGGL(border_bwd_kernel<false>, grid, block, 0, s, logits, target, d1sq, d2sq, out, dloss, dlogits, K, HW, bpi,
                           fg, ignore, inv2s2);
    return launch_status("border_bwd");
}

}  // namespace medt
