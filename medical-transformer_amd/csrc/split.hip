// split.hip -- splitting touching objects of a mask on the device: the marker pass of a marker-controlled growth and the growth
// itself (medt_split_* and medt_grow_* in medt_abi.h; medt_amd.ops.split_markers / grow_labels / split_objects; test.py --split;
// not in the reference, whose users run SciPy's distance transform and scikit-image's peak_local_max and watershed on the host).
//
// All integers, and every result is the same whatever order the work-items and workgroups run in:
//   split_cmax     cmax[n, l] = max of the squared depth over component l: integer atomicMax, reduced per workgroup in LDS first
//   split_marker   one workgroup per LABEL tile: the squared depths of the tile and its r-pixel halo in LDS (0 beyond the image),
//                  the (2r+1) x (2r+1) window maximum taken separably (rows, then columns), the int64 predicate
//                  sqrt(M) - sqrt(depth2) <= t  <=>  e <= 0 or e^2 <= 4 t^2 depth2  with e = M - depth2 - t^2,  OR depth2 == cmax
//   grow_pass      one packed key (distance << 32 | label) per pixel; one workgroup per tile loads the tile and a 1-pixel halo
//                  into LDS, relaxes key(p) = min(key(p), min over neighbours q of key(q) + (1 << 32)) in LDS until a sweep
//                  changes nothing, and stores its own pixels only.  Keys only ever decrease and never fall below the true
//                  (geodesic distance, smallest label at that distance), so a halo that another workgroup is still lowering costs
//                  a pass, never the result.  Nobody waits on another workgroup; the sweep loop is capped at the pixel count of
//                  tile plus halo.  A tile whose own and whose eight neighbours' keys did not change in the pass before exits at
//                  once (per-tile flags, double-buffered by the parity of the pass).
//   grow_unpack    labels = the key's low word where a seed was reached, else 0
// A key is 8 bytes, 8-byte aligned, and moves as one access: LDS reads and writes of a sweep are separated by barriers (Jacobi),
// global keys are read and written with relaxed atomic 64-bit accesses.  No float anywhere.
#include "medt_kernels.h"

namespace medt {

constexpr int SPLIT_TH = MEDT_LABEL_TILE_H, SPLIT_TW = MEDT_LABEL_TILE_W;
constexpr int SPLIT_CHUNK = 4 * MEDT_THREADS;             // pixels of a chunk of the linear passes
constexpr int SPLIT_R = MEDT_SPLIT_MAX_DISTANCE;          // the largest window radius: sizes the LDS of the marker pass
constexpr int SPLIT_SLOTS = MEDT_THREADS;
static_assert(SPLIT_TH * SPLIT_TW == 4 * MEDT_THREADS && SPLIT_TW % 4 == 0, "a work-item owns 4 neighbouring pixels of a tile row");
static_assert(((SPLIT_TH + 2 * SPLIT_R) * (SPLIT_TW + 2 * SPLIT_R) + (SPLIT_TH + 2 * SPLIT_R) * SPLIT_TW) * 4 <= 64 * 1024,
              "tile + halo and the row maxima fit the static LDS of a workgroup");

typedef unsigned long long grow_key;
constexpr grow_key GROW_OUTSIDE = ~0ull;                  // a pixel outside the mask (or outside the image)
constexpr grow_key GROW_FAR = 0x7FFFFFFFull << 32;        // a pixel of the mask no seed has reached (yet)
constexpr grow_key GROW_STEP = 1ull << 32;
constexpr int GROW_LW = SPLIT_TW + 2, GROW_LH = SPLIT_TH + 2;
constexpr int GROW_SWEEP_CAP = GROW_LW * GROW_LH;         // the pixel count of tile plus halo

#ifdef MEDT_LANE_EMU
// (atomicMax / atomicCAS on int: label.hip's stand-ins, which this translation unit follows in the emulated library)
template <class T> static inline void __hip_atomic_store(T* p, T v, int, int) { *p = v; }
#endif

__device__ __forceinline__ grow_key grow_ld(const grow_key* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void grow_st(grow_key* p, grow_key v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---- component maxima ------------------------------------------------------------------------------------------------------
// SPLIT_SLOTS direct-mapped LDS slots keyed by label % SPLIT_SLOTS, claimed with a compare-and-swap; a label that finds its
// slot taken goes to the global table directly (label_boxes_kernel's scheme).  A run of one label inside a work-item's four
// pixels is one update.  cmax starts at 0 (the host clears it); depths inside a component are >= 1.
__device__ __forceinline__ void split_cmax_put(int* owner, int* best, int32_t* __restrict__ gmax, int l, int d) {
    const int slot = l % SPLIT_SLOTS;
    const int old = atomicCAS(owner + slot, 0, l);
    if (old == 0 || old == l) atomicMax(best + slot, d);
    else atomicMax(gmax + l, d);
}

__global__ __launch_bounds__(MEDT_THREADS) void split_cmax_kernel(const int32_t* __restrict__ depth2, const int32_t* __restrict__ comp,
                                                                  int32_t* __restrict__ cmax, int HW, int cpi, int stride) {
    MEDT_STATIC_SHARED int owner[SPLIT_SLOTS];
    MEDT_STATIC_SHARED int best[SPLIT_SLOTS];
    const int n = blockIdx.x / cpi, p0 = (blockIdx.x - n * cpi) * SPLIT_CHUNK + threadIdx.x * 4;
    const size_t base = (size_t)n * HW;
    int32_t* gmax = cmax + (size_t)n * stride;
    owner[threadIdx.x] = 0;
    best[threadIdx.x] = 0;
    __syncthreads();
    int run_label = 0, run_max = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (p0 + e >= HW) break;
        const int l = comp[base + p0 + e];
        if (l < 1 || l >= stride) continue;
        const int d = depth2[base + p0 + e];
        if (l != run_label) {
            if (run_label) split_cmax_put(owner, best, gmax, run_label, run_max);
            run_label = l; run_max = d;
        } else {
            run_max = max(run_max, d);
        }
    }
    if (run_label) split_cmax_put(owner, best, gmax, run_label, run_max);
    __syncthreads();
    const int l = owner[threadIdx.x];
    if (l) atomicMax(gmax + l, best[threadIdx.x]);
}

int split_cmax(const int32_t* depth2, const int32_t* comp, int32_t* cmax, int N, int H, int W, int stride, hipStream_t s) {
    if (hipMemsetAsync(cmax, 0, (size_t)N * stride * sizeof(int32_t), s) != hipSuccess) {
        set_error("split_cmax: clearing the table failed"); return MEDT_ELAUNCH;
    }
    const int cpi = cdiv(H * W, SPLIT_CHUNK);
    hipLaunchKernelGGL(split_cmax_kernel, dim3((unsigned)N * cpi), dim3(MEDT_THREADS), 0, s, depth2, comp, cmax, H * W, cpi, stride);
    return launch_status("split_cmax");
}

// ---- markers ---------------------------------------------------------------------------------------------------------------
// stage: (SPLIT_TH + 2r) x (SPLIT_TW + 2r) squared depths, row pitch SPLIT_TW + 2r; rowmax: (SPLIT_TH + 2r) x SPLIT_TW maxima over
// the 2r + 1 columns around each pixel.  Every global index is formed from coordinates tested against the image first.
__global__ __launch_bounds__(MEDT_THREADS) void split_marker_kernel(const int32_t* __restrict__ depth2, const int32_t* __restrict__ comp,
                                                                    const int32_t* __restrict__ cmax, uint8_t* __restrict__ marker,
                                                                    int H, int W, int tiles_x, int tiles_y, int r, int t, int stride) {
    MEDT_STATIC_SHARED int stage[(SPLIT_TH + 2 * SPLIT_R) * (SPLIT_TW + 2 * SPLIT_R)];
    MEDT_STATIC_SHARED int rowmax[(SPLIT_TH + 2 * SPLIT_R) * SPLIT_TW];
    const int tile = blockIdx.x % (tiles_x * tiles_y), n = blockIdx.x / (tiles_x * tiles_y);
    const int y0 = (tile / tiles_x) * SPLIT_TH, x0 = (tile % tiles_x) * SPLIT_TW;
    const size_t base = (size_t)n * H * W;
    const int sh = SPLIT_TH + 2 * r, sw = SPLIT_TW + 2 * r, win = 2 * r + 1;
    for (int i = threadIdx.x; i < sh * sw; i += MEDT_THREADS) {
        const int gy = y0 - r + i / sw, gx = x0 - r + i % sw;
        stage[i] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? depth2[base + (size_t)gy * W + gx] : 0;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < sh * SPLIT_TW; i += MEDT_THREADS) {
        const int* row = stage + (i / SPLIT_TW) * sw + i % SPLIT_TW;
        int m = 0;
        for (int k = 0; k < win; ++k) m = max(m, row[k]);
        rowmax[i] = m;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SPLIT_TH * SPLIT_TW; i += MEDT_THREADS) {
        const int ly = i / SPLIT_TW, lx = i % SPLIT_TW, y = y0 + ly, x = x0 + lx;
        if (y >= H || x >= W) continue;
        const size_t p = base + (size_t)y * W + x;
        const int l = comp[p];
        uint8_t out = 0;
        if (l > 0) {
            int m = 0;
            for (int k = 0; k < win; ++k) m = max(m, rowmax[(ly + k) * SPLIT_TW + lx]);
            const long long d = stage[(ly + r) * sw + lx + r];
            const long long e = (long long)m - d - (long long)t * t;
            const bool near_top = e <= 0 || e * e <= 4ll * t * t * d;
            const bool comp_top = l < stride && d == (long long)cmax[(size_t)n * stride + l];
            out = (near_top || comp_top) ? 255 : 0;
        }
        marker[p] = out;
    }
}

int split_markers(const int32_t* depth2, const int32_t* comp, const int32_t* cmax, uint8_t* marker, int N, int H, int W, int stride,
                  int distance, int tolerance, hipStream_t s) {
    const int tiles_x = cdiv(W, SPLIT_TW), tiles_y = cdiv(H, SPLIT_TH);
    hipLaunchKernelGGL(split_marker_kernel, dim3((unsigned)N * tiles_x * tiles_y), dim3(MEDT_THREADS), 0, s, depth2, comp, cmax, marker,
                       H, W, tiles_x, tiles_y, distance, tolerance, stride);
    return launch_status("split_markers");
}

// ---- growth ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MEDT_THREADS) void grow_init_kernel(const int32_t* __restrict__ seeds, const uint8_t* __restrict__ mask,
                                                                 grow_key* __restrict__ keys, unsigned total) {
    const unsigned i = blockIdx.x * MEDT_THREADS + threadIdx.x;
    if (i >= total) return;
    const int sd = seeds[i];
    keys[i] = mask[i] == 0 ? GROW_OUTSIDE : (sd > 0 ? (grow_key)(uint32_t)sd : GROW_FAR);
}

__device__ __forceinline__ grow_key grow_relax(grow_key best, grow_key q) { return q < GROW_FAR ? min(best, q + GROW_STEP) : best; }

// Work-item t owns the pixels (t / 16, 4 (t % 16) .. + 3) of the tile.  flag_prev / flag_cur: one int32 per tile, != 0 when the
// tile's keys changed in the pass before / in this pass; changed: one int32 of this pass, raised by every tile that changed.
template <bool CONN8>
__global__ __launch_bounds__(MEDT_THREADS) void grow_pass_kernel(grow_key* __restrict__ keys, const int32_t* __restrict__ flag_prev,
                                                                 int32_t* __restrict__ flag_cur, int32_t* __restrict__ changed,
                                                                 int H, int W, int tiles_x, int tiles_y) {
    MEDT_STATIC_SHARED grow_key lk[GROW_LH * GROW_LW];
    MEDT_STATIC_SHARED int sweep_flag[2];
    MEDT_STATIC_SHARED int tile_changed;
    const int tpi = tiles_x * tiles_y, tile = blockIdx.x % tpi, n = blockIdx.x / tpi;
    const int ty = tile / tiles_x, tx = tile % tiles_x;
    int active = 0;                                        // (the flags of the pass before: nothing writes them in this launch)
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int yy = ty + dy, xx = tx + dx;
            if (yy >= 0 && yy < tiles_y && xx >= 0 && xx < tiles_x) active |= flag_prev[(size_t)n * tpi + yy * tiles_x + xx];
        }
    if (!active) {                                         // (uniform over the workgroup: nobody is left at a barrier)
        if (threadIdx.x == 0) flag_cur[blockIdx.x] = 0;
        return;
    }
    const int y0 = ty * SPLIT_TH, x0 = tx * SPLIT_TW;
    grow_key* img = keys + (size_t)n * H * W;
    for (int i = threadIdx.x; i < GROW_LH * GROW_LW; i += MEDT_THREADS) {
        const int gy = y0 - 1 + i / GROW_LW, gx = x0 - 1 + i % GROW_LW;
        lk[i] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? grow_ld(img + (size_t)gy * W + gx) : GROW_OUTSIDE;
    }
    if (threadIdx.x == 0) { sweep_flag[0] = 0; sweep_flag[1] = 0; tile_changed = 0; }
    __syncthreads();
    const int ly = threadIdx.x / (SPLIT_TW / 4), lx = (threadIdx.x % (SPLIT_TW / 4)) * 4;
    const int c0 = (ly + 1) * GROW_LW + lx + 1;
    grow_key first[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) first[e] = lk[c0 + e];
    bool settled = false;
    for (int sweep = 0; sweep < GROW_SWEEP_CAP; ++sweep) {
        grow_key nk[4];
        bool lower = false;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = c0 + e;
            const grow_key k = lk[i];
            grow_key b = k;
            if (k != GROW_OUTSIDE) {
                b = grow_relax(b, lk[i - 1]);
                b = grow_relax(b, lk[i + 1]);
                b = grow_relax(b, lk[i - GROW_LW]);
                b = grow_relax(b, lk[i + GROW_LW]);
                if (CONN8) {
                    b = grow_relax(b, lk[i - GROW_LW - 1]);
                    b = grow_relax(b, lk[i - GROW_LW + 1]);
                    b = grow_relax(b, lk[i + GROW_LW - 1]);
                    b = grow_relax(b, lk[i + GROW_LW + 1]);
                }
            }
            nk[e] = b;
            lower |= b < k;
        }
        __syncthreads();                                   // every read of this sweep is done
        if (threadIdx.x == 0) sweep_flag[(sweep + 1) & 1] = 0;
        if (lower) {
#pragma unroll
            for (int e = 0; e < 4; ++e) lk[c0 + e] = nk[e];
            sweep_flag[sweep & 1] = 1;
        }
        __syncthreads();
        if (!sweep_flag[sweep & 1]) { settled = true; break; }     // (uniform: one LDS word, read behind the barrier)
    }
    bool mine = !settled;                                  // a tile that hit the cap writes what it has and reports "changed"
    const int y = y0 + ly;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const grow_key k = lk[c0 + e];
        if (k != first[e]) {                               // (a changed key was inside the mask, hence inside the image)
            mine = true;
            if (y < H && x0 + lx + e < W) grow_st(img + (size_t)y * W + x0 + lx + e, k);
        }
    }
    if (mine) tile_changed = 1;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int c = tile_changed;
        flag_cur[blockIdx.x] = c;
        if (c) atomicMax(changed, 1);
    }
}

__global__ __launch_bounds__(MEDT_THREADS) void grow_unpack_kernel(const grow_key* __restrict__ keys, int32_t* __restrict__ labels,
                                                                   int32_t* __restrict__ dist, unsigned total) {
    const unsigned i = blockIdx.x * MEDT_THREADS + threadIdx.x;
    if (i >= total) return;
    const grow_key k = keys[i];
    const bool reached = k < GROW_FAR;
    labels[i] = reached ? (int32_t)(uint32_t)(k & 0xFFFFFFFFull) : 0;
    if (dist) dist[i] = reached ? (int32_t)(k >> 32) : -1;
}

static inline int grow_tiles(int H, int W) { return cdiv(W, SPLIT_TW) * cdiv(H, SPLIT_TH); }
static inline size_t grow_keys_bytes(int N, int H, int W) { return align_up((size_t)N * H * W * sizeof(grow_key), 256); }

size_t grow_workspace_bytes(int N, int H, int W) {
    return align_up(grow_keys_bytes(N, H, W) + (size_t)2 * N * grow_tiles(H, W) * sizeof(int32_t), 16);
}

int grow_init(const int32_t* seeds, const uint8_t* mask, void* workspace, int N, int H, int W, hipStream_t s) {
    grow_key* keys = (grow_key*)workspace;
    int32_t* flags = (int32_t*)((char*)workspace + grow_keys_bytes(N, H, W));
    // every tile counts as changed in front of the first pass (any non-zero word)
    if (hipMemsetAsync(flags, 1, (size_t)2 * N * grow_tiles(H, W) * sizeof(int32_t), s) != hipSuccess) {
        set_error("grow_init: setting the tile flags failed"); return MEDT_ELAUNCH;
    }
    const unsigned total = (unsigned)((size_t)N * H * W);
    hipLaunchKernelGGL(grow_init_kernel, dim3((total + MEDT_THREADS - 1) / MEDT_THREADS), dim3(MEDT_THREADS), 0, s, seeds, mask, keys, total);
    return launch_status("grow_init");
}

int grow_passes(void* workspace, int32_t* changed, int n_passes, int first_pass, int N, int H, int W, int connectivity, hipStream_t s) {
    grow_key* keys = (grow_key*)workspace;
    int32_t* flags = (int32_t*)((char*)workspace + grow_keys_bytes(N, H, W));
    if (hipMemsetAsync(changed, 0, (size_t)n_passes * sizeof(int32_t), s) != hipSuccess) {
        set_error("grow_passes: clearing the pass flags failed"); return MEDT_ELAUNCH;
    }
    const int tiles_x = cdiv(W, SPLIT_TW), tiles_y = cdiv(H, SPLIT_TH);
    const size_t tiles = (size_t)N * tiles_x * tiles_y;
    const dim3 grid((unsigned)tiles), block(MEDT_THREADS);
    for (int i = 0; i < n_passes; ++i) {
        const int par = (first_pass + i) & 1;
        int32_t* cur = flags + par * tiles;
        const int32_t* prev = flags + (par ^ 1) * tiles;
        if (connectivity == 8) hipLaunchKernelGGL((grow_pass_kernel<true>), grid, block, 0, s, keys, prev, cur, changed + i, H, W, tiles_x, tiles_y);
        else hipLaunchKernelGGL((grow_pass_kernel<false>), grid, block, 0, s, keys, prev, cur, changed + i, H, W, tiles_x, tiles_y);
    }
    return launch_status("grow_passes");
}

int grow_unpack(const void* workspace, int32_t* labels, int32_t* dist, int N, int H, int W, hipStream_t s) {
    const unsigned total = (unsigned)((size_t)N * H * W);
    hipLaunchKernelGGL(grow_unpack_kernel, dim3((total + MEDT_THREADS - 1) / MEDT_THREADS), dim3(MEDT_THREADS), 0, s,
                       (const grow_key*)workspace, labels, dist, total);
    return launch_status("grow_unpack");
}

}  // namespace medt
