// label.hip -- connected-component labelling of uint8 masks on the device, the per-component tables and the table-driven
// select pass (medt_label_* in medt_abi.h; medt_amd.ops.label / label_tables / remove_small_objects / fill_holes,
// metrics.object_scores: object-level F1 and Dice, AJI, PQ; not in the reference, whose users label on the host), and further
// down the bounding boxes of the components and the directed squared Hausdorff distances of pairs of them (medt_label_boxes,
// medt_pair_hausdorff; metrics.object_hausdorff: the object-level Hausdorff distance of GlaS).
//
// Labelling is a union-find over the pixels of the labelled set (mask != 0, or mask == 0 in background mode); a node's parent
// is always a pixel index that is not larger than its own, so every chain of parents strictly decreases and ends in the
// SMALLEST index of its set -- whatever order concurrent unions land in.  Six launches, nothing waits on another workgroup:
//   1 label_local    one workgroup per LABEL_TH x LABEL_TW tile: union-find in LDS over the pairs inside the tile, then
//                    parent[pixel] = batch-linear index of the tile-local root (-1 outside the labelled set)
//   2 label_border   one work-item per pixel next to a tile edge: unions across the edge (8-connectivity: the diagonal pairs
//                    too, which covers the pairs across tile corners) by atomicMin on the parent map
//   3 label_flatten  root[pixel] = end of the pixel's parent chain (into the labels array), roots per 1024-pixel chunk counted
//   4 label_scan     one workgroup per image: exclusive scan of the chunk counts in a fixed order, count[n] = their sum
//   5 label_rank     parent[root] = chunk offset + roots in front of it in the chunk + 1: its rank in raster order
//   6 label_apply    labels[pixel] = parent[root[pixel]], 0 outside the labelled set
// All integers; the ranks are a prefix sum in a fixed order: the labels are those of scipy.ndimage.label bit for bit, on every run.
#include "medt_kernels.h"

namespace medt {

constexpr int LABEL_TH = MEDT_LABEL_TILE_H, LABEL_TW = MEDT_LABEL_TILE_W;
constexpr int LABEL_TILE = LABEL_TH * LABEL_TW;          // pixels of a tile = 4 per work-item
constexpr int LABEL_CHUNK = 4 * MEDT_THREADS;            // pixels of a chunk of the linear passes
static_assert(LABEL_TILE == 4 * MEDT_THREADS && LABEL_TW % 4 == 0, "a work-item owns 4 neighbouring pixels of a tile row");

struct alignas(16) LabelQuad {
    int32_t v[4];
};

#ifdef MEDT_LANE_EMU
// The CPU lane emulator's HIP vocabulary (tests/lane_emu) has atomicAdd and atomicOr but no atomicMin.  One work-item runs at
// a time there, so a read-modify-write is atomic by construction.
static inline int atomicMin(int* p, int v) { const int o = *p; *p = o < v ? o : v; return o; }
static inline int atomicMax(int* p, int v) { const int o = *p; *p = o > v ? o : v; return o; }
static inline int atomicCAS(int* p, int expected, int v) { const int o = *p; if (o == expected) *p = v; return o; }
#endif

// A parent that another work-item may be changing in the same launch: never from a register copy or (global memory) from
// another XCD's L2.  For LDS the scope costs nothing.
__device__ __forceinline__ int label_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int label_find(const int* p, int x) {
    for (;;) {
        const int q = label_ld(p + x);      // q <= x always: the walk ends
        if (q == x) return x;
        x = q;
    }
}

// Unite the sets of a and b.  The larger of the two candidate roots is pointed at the smaller with atomicMin.  When the
// node turns out not to be a root any more (another union got there first) atomicMin returns its earlier parent `old` < a:
// the link a -> old was either kept (old <= b) or replaced by a -> b, and in both cases uniting old with b restores what is
// missing.  max(a, b) strictly decreases from one round to the next, so the loop ends by its own progress.
__device__ __forceinline__ void label_union(int* p, int a, int b) {
    for (;;) {
        a = label_find(p, a);
        b = label_find(p, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(p + a, b);
        if (old == a) return;
        a = old;
    }
}

template <int CPT>
__device__ __forceinline__ void label_load_i32(const int32_t* __restrict__ p, int (&a)[CPT]) {
    if (CPT == 4) {
        const LabelQuad q = *reinterpret_cast<const LabelQuad*>(p);
#pragma unroll
        for (int e = 0; e < CPT; ++e) a[e] = q.v[e];
    } else {
        a[0] = p[0];
    }
}
template <int CPT>
__device__ __forceinline__ void label_store_i32(int32_t* __restrict__ p, const int (&a)[CPT]) {
    if (CPT == 4) {
        LabelQuad q;
#pragma unroll
        for (int e = 0; e < CPT; ++e) q.v[e] = a[e];
        *reinterpret_cast<LabelQuad*>(p) = q;
    } else {
        p[0] = a[0];
    }
}

// ---- 1. tiles ------------------------------------------------------------------------------------------------------------
// Work-item t owns the pixels (t / 16, 4 (t % 16) .. + 3) of the tile.  VEC: W % 4 == 0 and aligned pointers, so a quad is
// inside the image as a whole or not at all and moves as one 4-byte load and one 16-byte store.
template <bool VEC, bool CONN8>
__global__ __launch_bounds__(MEDT_THREADS) void label_local_kernel(const uint8_t* __restrict__ mask, int32_t* __restrict__ parent,
                                                                   int H, int W, int tiles_x, int tiles_y, int background) {
    MEDT_STATIC_SHARED int lp[LABEL_TILE];
    const int tile = blockIdx.x % (tiles_x * tiles_y), n = blockIdx.x / (tiles_x * tiles_y);
    const int y0 = (tile / tiles_x) * LABEL_TH, x0 = (tile % tiles_x) * LABEL_TW;
    const int ly = threadIdx.x / (LABEL_TW / 4), lx = (threadIdx.x % (LABEL_TW / 4)) * 4;
    const int y = y0 + ly, x = x0 + lx, i0 = ly * LABEL_TW + lx;
    const size_t base = (size_t)n * H * W;
    uint32_t set = 0;                                     // bit e: pixel x + e belongs to the labelled set
    if (y < H) {
        const uint8_t* row = mask + base + (size_t)y * W;
        if (VEC) {
            if (x < W) {
                const uint32_t w = *reinterpret_cast<const uint32_t*>(row + x);
#pragma unroll
                for (int e = 0; e < 4; ++e) set |= ((((w >> (8 * e)) & 255u) != 0) != (background != 0)) ? 1u << e : 0u;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (x + e < W) set |= ((row[x + e] != 0) != (background != 0)) ? 1u << e : 0u;
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) lp[i0 + e] = ((set >> e) & 1u) ? i0 + e : -1;
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (!((set >> e) & 1u)) continue;
        const int i = i0 + e, cx = lx + e;
        if (cx > 0 && label_ld(lp + i - 1) >= 0) label_union(lp, i, i - 1);   // (membership, the sign, never changes)
        if (ly > 0) {
            if (label_ld(lp + i - LABEL_TW) >= 0) label_union(lp, i, i - LABEL_TW);
            if (CONN8) {
                if (cx > 0 && label_ld(lp + i - LABEL_TW - 1) >= 0) label_union(lp, i, i - LABEL_TW - 1);
                if (cx < LABEL_TW - 1 && label_ld(lp + i - LABEL_TW + 1) >= 0) label_union(lp, i, i - LABEL_TW + 1);
            }
        }
    }
    __syncthreads();
    if (y >= H || x >= W) return;
    int out[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        out[e] = -1;
        if ((set >> e) & 1u) {
            const int r = label_find(lp, i0 + e);          // tile order = raster order inside the tile: the smallest index of both
            out[e] = (int)(base + (size_t)(y0 + r / LABEL_TW) * W + (x0 + r % LABEL_TW));
        }
    }
    int32_t* dst = parent + base + (size_t)y * W + x;
    if (VEC) {
        label_store_i32<4>(dst, out);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (x + e < W) dst[e] = out[e];
    }
}

// ---- 2. tile edges -------------------------------------------------------------------------------------------------------
// Per image: rows_b horizontal tile edges of W pixels each (the pixel below the edge looks up), then cols_b vertical ones of
// H pixels each (the pixel right of the edge looks left).  With 8-connectivity each also looks along its two diagonals across
// the edge; where four tiles meet both diagonals are among them.
template <bool CONN8>
__global__ __launch_bounds__(MEDT_THREADS) void label_border_kernel(int32_t* __restrict__ parent, int H, int W, int rows_b, int cols_b,
                                                                    int per_image, int total) {
    const int item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= total) return;
    const int n = item / per_image, k = item - n * per_image;
    const int base = n * H * W;
    int y, x, dy0, dx0;                                   // the neighbour straight across the edge is (y + dy0, x + dx0)
    if (k < rows_b * W) {
        y = (k / W + 1) * LABEL_TH; x = k % W; dy0 = -1; dx0 = 0;
    } else {
        const int c = k - rows_b * W;
        x = (c / H + 1) * LABEL_TW; y = c % H; dy0 = 0; dx0 = -1;
    }
    const int me = base + y * W + x;
    if (label_ld(parent + me) < 0) return;
#pragma unroll
    for (int s = -1; s <= 1; ++s) {
        if (s != 0 && !CONN8) continue;
        const int yy = y + dy0 + (dx0 ? s : 0), xx = x + dx0 + (dy0 ? s : 0);
        if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
        const int other = base + yy * W + xx;
        if (label_ld(parent + other) >= 0) label_union(parent, me, other);
    }
}

// ---- 3..6. roots, their ranks, the labels ----------------------------------------------------------------------------------
// The linear passes: an image is cut into chunks of LABEL_CHUNK pixels in raster order, one workgroup each; work-item t owns
// the pixels 4t .. 4t + 3 of the chunk, so work-item order is raster order.  VEC: they move as one 16-byte access (W % 4 == 0
// and aligned pointers); otherwise one element at a time.
template <bool VEC>
__global__ __launch_bounds__(MEDT_THREADS) void label_flatten_kernel(const int32_t* __restrict__ parent, int32_t* __restrict__ root,
                                                                     int32_t* __restrict__ partial, int HW, int cpi) {
    MEDT_STATIC_SHARED int roots;
    const int n = blockIdx.x / cpi, p0 = (blockIdx.x - n * cpi) * LABEL_CHUNK + threadIdx.x * 4;
    const size_t base = (size_t)n * HW;
    if (threadIdx.x == 0) roots = 0;
    __syncthreads();
    int mine = 0;
    if (p0 < HW) {
        int a[4] = {-1, -1, -1, -1};
        if (VEC) {
            label_load_i32<4>(parent + base + p0, a);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (p0 + e < HW) a[e] = parent[base + p0 + e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (a[e] < 0) continue;
            const int self = (int)base + p0 + e;
            mine += a[e] == self;
            int r = a[e];
            for (int q = parent[r]; q != r; q = parent[r]) r = q;          // (nothing writes the parent map in this launch)
            a[e] = r;
        }
        if (VEC) {
            label_store_i32<4>(root + base + p0, a);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (p0 + e < HW) root[base + p0 + e] = a[e];
        }
    }
    if (mine) atomicAdd(&roots, mine);                     // (an integer sum: the order does not matter)
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = roots;
}

// One workgroup per image; work-item t scans the chunk counts [t seg, (t + 1) seg) serially, the 256 segment sums are scanned
// by work-item 0: a fixed order.  partial becomes the exclusive scan.
__global__ __launch_bounds__(MEDT_THREADS) void label_scan_kernel(int32_t* __restrict__ partial, int32_t* __restrict__ count, int cpi) {
    MEDT_STATIC_SHARED int seg_sum[MEDT_THREADS];
    int32_t* p = partial + (size_t)blockIdx.x * cpi;
    const int seg = (cpi + MEDT_THREADS - 1) / MEDT_THREADS;
    const int lo = min((int)threadIdx.x * seg, cpi), hi = min(lo + seg, cpi);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += p[i];
    seg_sum[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int t = 0; t < MEDT_THREADS; ++t) { const int v = seg_sum[t]; seg_sum[t] = run; run += v; }
        count[blockIdx.x] = run;
    }
    __syncthreads();
    int run = seg_sum[threadIdx.x];
    for (int i = lo; i < hi; ++i) { const int v = p[i]; p[i] = run; run += v; }
}

// parent[root] = rank of the root among the roots of its image, from 1, in raster order.  Every work-item reads and writes its
// own four pixels of the parent map only.
template <bool VEC>
__global__ __launch_bounds__(MEDT_THREADS) void label_rank_kernel(int32_t* __restrict__ parent, const int32_t* __restrict__ partial,
                                                                  int HW, int cpi) {
    MEDT_STATIC_SHARED int scan[2][MEDT_THREADS];
    const int n = blockIdx.x / cpi, p0 = (blockIdx.x - n * cpi) * LABEL_CHUNK + threadIdx.x * 4;
    const size_t base = (size_t)n * HW;
    int a[4] = {-1, -1, -1, -1};
    if (p0 < HW) {
        if (VEC) {
            label_load_i32<4>(parent + base + p0, a);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (p0 + e < HW) a[e] = parent[base + p0 + e];
        }
    }
    uint32_t is_root = 0;
    int mine = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (a[e] == (int)base + p0 + e) { is_root |= 1u << e; ++mine; }
    // inclusive scan of the 256 per-work-item counts (Hillis-Steele, double-buffered)
    int cur = 0;
    scan[0][threadIdx.x] = mine;
    __syncthreads();
    for (int d = 1; d < MEDT_THREADS; d <<= 1) {
        int v = scan[cur][threadIdx.x];
        if ((int)threadIdx.x >= d) v += scan[cur][threadIdx.x - d];
        scan[cur ^ 1][threadIdx.x] = v;
        cur ^= 1;
        __syncthreads();
    }
    if (!is_root) return;
    int rank = partial[blockIdx.x] + scan[cur][threadIdx.x] - mine;
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if ((is_root >> e) & 1u) parent[base + p0 + e] = ++rank;
}

template <bool VEC>
__global__ __launch_bounds__(MEDT_THREADS) void label_apply_kernel(const int32_t* __restrict__ parent, int32_t* __restrict__ labels,
                                                                   int HW, int cpi) {
    const int n = blockIdx.x / cpi, p0 = (blockIdx.x - n * cpi) * LABEL_CHUNK + threadIdx.x * 4;
    const size_t base = (size_t)n * HW;
    if (p0 >= HW) return;
    int a[4] = {-1, -1, -1, -1};
    if (VEC) {
        label_load_i32<4>(labels + base + p0, a);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (p0 + e < HW) a[e] = labels[base + p0 + e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] = a[e] < 0 ? 0 : parent[a[e]];
    if (VEC) {
        label_store_i32<4>(labels + base + p0, a);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (p0 + e < HW) labels[base + p0 + e] = a[e];
    }
}

static inline int label_chunks(int H, int W) { return cdiv(H * W, LABEL_CHUNK); }

size_t label_workspace_bytes(int N, int H, int W) {
    return align_up((size_t)N * H * W * sizeof(int32_t), 256) + (size_t)N * label_chunks(H, W) * sizeof(int32_t);
}

int label_components(const uint8_t* mask, int32_t* labels, int32_t* count, void* workspace, int N, int H, int W, int connectivity,
                     int background, hipStream_t s) {
    int32_t* parent = (int32_t*)workspace;
    int32_t* partial = (int32_t*)((char*)workspace + align_up((size_t)N * H * W * sizeof(int32_t), 256));
    const bool vec = (W % 4 == 0) && ((uintptr_t)mask % 4 == 0) && ((uintptr_t)parent % 16 == 0) && ((uintptr_t)labels % 16 == 0);
    const bool c8 = connectivity == 8;
    const int tiles_x = cdiv(W, LABEL_TW), tiles_y = cdiv(H, LABEL_TH), cpi = label_chunks(H, W), HW = H * W;
    const dim3 block(MEDT_THREADS), tiles((unsigned)N * tiles_x * tiles_y), chunks((unsigned)N * cpi);
#define MEDT_LABEL_LOCAL(VV, CC) \
    hipLaunchKernelGGL((label_local_kernel<VV, CC>), tiles, block, 0, s, mask, parent, H, W, tiles_x, tiles_y, background)
    if (vec) {
        if (c8) MEDT_LABEL_LOCAL(true, true); else MEDT_LABEL_LOCAL(true, false);
    } else {
        if (c8) MEDT_LABEL_LOCAL(false, true); else MEDT_LABEL_LOCAL(false, false);
    }
#undef MEDT_LABEL_LOCAL
    const int rows_b = tiles_y - 1, cols_b = tiles_x - 1, per_image = rows_b * W + cols_b * H;
    if (per_image > 0) {
        const int total = N * per_image;                       // < 2 N H W / 16 < 2^31
        const dim3 grid((unsigned)cdiv(total, MEDT_THREADS));
        if (c8) hipLaunchKernelGGL((label_border_kernel<true>), grid, block, 0, s, parent, H, W, rows_b, cols_b, per_image, total);
        else hipLaunchKernelGGL((label_border_kernel<false>), grid, block, 0, s, parent, H, W, rows_b, cols_b, per_image, total);
    }
    if (vec) hipLaunchKernelGGL((label_flatten_kernel<true>), chunks, block, 0, s, parent, labels, partial, HW, cpi);
    else hipLaunchKernelGGL((label_flatten_kernel<false>), chunks, block, 0, s, parent, labels, partial, HW, cpi);
    hipLaunchKernelGGL(label_scan_kernel, dim3((unsigned)N), block, 0, s, partial, count, cpi);
    if (vec) hipLaunchKernelGGL((label_rank_kernel<true>), chunks, block, 0, s, parent, partial, HW, cpi);
    else hipLaunchKernelGGL((label_rank_kernel<false>), chunks, block, 0, s, parent, partial, HW, cpi);
    if (vec) hipLaunchKernelGGL((label_apply_kernel<true>), chunks, block, 0, s, parent, labels, HW, cpi);
    else hipLaunchKernelGGL((label_apply_kernel<false>), chunks, block, 0, s, parent, labels, HW, cpi);
    return launch_status("label_components");
}

// ---- component tables --------------------------------------------------------------------------------------------------------
// area[n, l] = pixels of label l (slot 0: the unlabelled rest), frame[n, l] = 1 when l touches the image's frame.  Integer
// atomics on the table; the unlabelled pixels, which would all meet at one address, are summed per workgroup in LDS first; a
// run of one label inside a work-item's four pixels is one atomic.  frame receives plain byte stores of the value 1.  A label
// outside [0, stride) is not counted (the host has refused a stride that cannot hold the counts).
template <bool VEC>
__global__ __launch_bounds__(MEDT_THREADS) void label_tables_kernel(const int32_t* __restrict__ labels, int32_t* __restrict__ area,
                                                                    uint8_t* __restrict__ frame, int H, int W, int cpi, int stride) {
    MEDT_STATIC_SHARED int rest;
    const int HW = H * W;
    const int n = blockIdx.x / cpi, p0 = (blockIdx.x - n * cpi) * LABEL_CHUNK + threadIdx.x * 4;
    const size_t base = (size_t)n * HW;
    if (threadIdx.x == 0) rest = 0;
    __syncthreads();
    if (p0 < HW) {
        int a[4] = {-1, -1, -1, -1};
        if (VEC) {
            label_load_i32<4>(labels + base + p0, a);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (p0 + e < HW) a[e] = labels[base + p0 + e];
        }
        int zeros = 0, run_label = -1, run = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int l = a[e];
            if (p0 + e >= HW || l < 0 || l >= stride) continue;
            if (l == 0) { ++zeros; continue; }
            const int y = (p0 + e) / W, x = (p0 + e) - y * W;
            if (y == 0 || y == H - 1 || x == 0 || x == W - 1) frame[(size_t)n * stride + l] = 1;
            if (l != run_label) {
                if (run) atomicAdd(area + (size_t)n * stride + run_label, run);
                run_label = l; run = 0;
            }
            ++run;
        }
        if (run) atomicAdd(area + (size_t)n * stride + run_label, run);
        if (zeros) atomicAdd(&rest, zeros);
    }
    __syncthreads();
    if (threadIdx.x == 0 && rest) atomicAdd(area + (size_t)n * stride, rest);
}

int label_tables(const int32_t* labels, int32_t* area, uint8_t* frame, int N, int H, int W, int stride, hipStream_t s) {
    if (hipMemsetAsync(area, 0, (size_t)N * stride * sizeof(int32_t), s) != hipSuccess ||
        hipMemsetAsync(frame, 0, (size_t)N * stride, s) != hipSuccess) {
        set_error("label_tables: clearing the tables failed"); return MEDT_ELAUNCH;
    }
    const bool vec = (W % 4 == 0) && ((uintptr_t)labels % 16 == 0);
    const int cpi = label_chunks(H, W);
    const dim3 grid((unsigned)N * cpi), block(MEDT_THREADS);
    if (vec) hipLaunchKernelGGL((label_tables_kernel<true>), grid, block, 0, s, labels, area, frame, H, W, cpi, stride);
    else hipLaunchKernelGGL((label_tables_kernel<false>), grid, block, 0, s, labels, area, frame, H, W, cpi, stride);
    return launch_status("label_tables");
}

// ---- select ------------------------------------------------------------------------------------------------------------------
// out = 255 where keep[n, labels] != 0 or (with_mask) mask != 0, else 0.
template <bool VEC>
__global__ __launch_bounds__(MEDT_THREADS) void label_select_kernel(const int32_t* __restrict__ labels, const uint8_t* __restrict__ keep,
                                                                    const uint8_t* __restrict__ mask, uint8_t* __restrict__ out,
                                                                    int HW, int cpi, int stride) {
    const int n = blockIdx.x / cpi, p0 = (blockIdx.x - n * cpi) * LABEL_CHUNK + threadIdx.x * 4;
    const size_t base = (size_t)n * HW;
    if (p0 >= HW) return;
    const uint8_t* k = keep + (size_t)n * stride;
    if (VEC) {
        int a[4];
        label_load_i32<4>(labels + base + p0, a);
        const uint32_t m = mask ? *reinterpret_cast<const uint32_t*>(mask + base + p0) : 0u;
        uint32_t w = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool on = (a[e] >= 0 && a[e] < stride && k[a[e]] != 0) || ((m >> (8 * e)) & 255u) != 0;
            w |= on ? 255u << (8 * e) : 0u;
        }
        *reinterpret_cast<uint32_t*>(out + base + p0) = w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (p0 + e >= HW) break;
            const int l = labels[base + p0 + e];
            const bool on = (l >= 0 && l < stride && k[l] != 0) || (mask && mask[base + p0 + e] != 0);
            out[base + p0 + e] = on ? 255 : 0;
        }
    }
}

int label_select(const int32_t* labels, const uint8_t* keep, const uint8_t* mask, uint8_t* out, int N, int H, int W, int stride,
                 hipStream_t s) {
    const bool vec = (W % 4 == 0) && ((uintptr_t)labels % 16 == 0) && ((uintptr_t)out % 4 == 0) && (!mask || (uintptr_t)mask % 4 == 0);
    const int cpi = label_chunks(H, W);
    const dim3 grid((unsigned)N * cpi), block(MEDT_THREADS);
    if (vec) hipLaunchKernelGGL((label_select_kernel<true>), grid, block, 0, s, labels, keep, mask, out, H * W, cpi, stride);
    else hipLaunchKernelGGL((label_select_kernel<false>), grid, block, 0, s, labels, keep, mask, out, H * W, cpi, stride);
    return launch_status("label_select");
}

// ---- bounding boxes ----------------------------------------------------------------------------------------------------------
// box[n, l] = (y0, x0, y1, x1), inclusive, of label l >= 1; (H, W, -1, -1) for a label without a pixel (what the init kernel
// writes into every slot; slot 0 is never touched again).  Integer atomicMin / atomicMax only, so the order does not matter.
// Per workgroup the boxes are first reduced in LDS: BOX_SLOTS direct-mapped slots keyed by label % BOX_SLOTS, claimed with a
// compare-and-swap; a label that finds its slot taken by another label goes to the global table directly.  Nobody waits:
// losing the claim is an answer, not a retry.  A run of one label inside a work-item's four pixels is one update.
constexpr int BOX_SLOTS = MEDT_THREADS;

__global__ __launch_bounds__(MEDT_THREADS) void label_boxes_init_kernel(int32_t* __restrict__ box, int H, int W, int total) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;      // one int32 of the (N, stride, 4) table
    if (i < total) box[i] = (i & 3) == 0 ? H : ((i & 3) == 1 ? W : -1);
}

__device__ __forceinline__ void label_box_put(int* owner, int (*lb)[BOX_SLOTS], int32_t* __restrict__ gbox, int l, int y0, int x0,
                                              int y1, int x1) {
    const int slot = l % BOX_SLOTS;
    const int old = atomicCAS(owner + slot, 0, l);
    if (old == 0 || old == l) {
        atomicMin(&lb[0][slot], y0); atomicMin(&lb[1][slot], x0); atomicMax(&lb[2][slot], y1); atomicMax(&lb[3][slot], x1);
    } else {
        int32_t* b = gbox + (size_t)l * 4;
        atomicMin(b + 0, y0); atomicMin(b + 1, x0); atomicMax(b + 2, y1); atomicMax(b + 3, x1);
    }
}

template <bool VEC>
__global__ __launch_bounds__(MEDT_THREADS) void label_boxes_kernel(const int32_t* __restrict__ labels, int32_t* __restrict__ box,
                                                                   int H, int W, int cpi, int stride) {
    MEDT_STATIC_SHARED int owner[BOX_SLOTS];
    MEDT_STATIC_SHARED int lb[4][BOX_SLOTS];
    const int HW = H * W;
    const int n = blockIdx.x / cpi, p0 = (blockIdx.x - n * cpi) * LABEL_CHUNK + threadIdx.x * 4;
    const size_t base = (size_t)n * HW;
    int32_t* gbox = box + (size_t)n * stride * 4;
    owner[threadIdx.x] = 0;
    lb[0][threadIdx.x] = H; lb[1][threadIdx.x] = W; lb[2][threadIdx.x] = -1; lb[3][threadIdx.x] = -1;
    __syncthreads();
    if (p0 < HW) {
        int a[4] = {-1, -1, -1, -1};
        if (VEC) {
            label_load_i32<4>(labels + base + p0, a);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (p0 + e < HW) a[e] = labels[base + p0 + e];
        }
        int run_label = 0, y0 = 0, x0 = 0, y1 = 0, x1 = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int l = a[e];
            if (p0 + e >= HW || l < 1 || l >= stride) continue;
            const int y = (p0 + e) / W, x = (p0 + e) - y * W;
            if (l != run_label) {
                if (run_label) label_box_put(owner, lb, gbox, run_label, y0, x0, y1, x1);
                run_label = l; y0 = y1 = y; x0 = x1 = x;
            } else {
                y0 = min(y0, y); y1 = max(y1, y); x0 = min(x0, x); x1 = max(x1, x);
            }
        }
        if (run_label) label_box_put(owner, lb, gbox, run_label, y0, x0, y1, x1);
    }
    __syncthreads();
    const int l = owner[threadIdx.x];
    if (l) {
        int32_t* b = gbox + (size_t)l * 4;
        atomicMin(b + 0, lb[0][threadIdx.x]); atomicMin(b + 1, lb[1][threadIdx.x]);
        atomicMax(b + 2, lb[2][threadIdx.x]); atomicMax(b + 3, lb[3][threadIdx.x]);
    }
}

int label_boxes(const int32_t* labels, int32_t* box, int N, int H, int W, int stride, hipStream_t s) {
    const dim3 block(MEDT_THREADS);
    const int total = N * stride * 4;                          // (the host has refused a table of 2^31 int32 or more)
    hipLaunchKernelGGL(label_boxes_init_kernel, dim3((unsigned)cdiv(total, MEDT_THREADS)), block, 0, s, box, H, W, total);
    const bool vec = (W % 4 == 0) && ((uintptr_t)labels % 16 == 0);
    const int cpi = label_chunks(H, W);
    const dim3 grid((unsigned)N * cpi);
    if (vec) hipLaunchKernelGGL((label_boxes_kernel<true>), grid, block, 0, s, labels, box, H, W, cpi, stride);
    else hipLaunchKernelGGL((label_boxes_kernel<false>), grid, block, 0, s, labels, box, H, W, cpi, stride);
    return launch_status("label_boxes");
}

// ---- directed squared Hausdorff distances of pairs of components ----------------------------------------------------------------
// A JOB is one pair and one direction: a query object (label q of one map) and a feature object (label f of the other).  Its
// result, max over the query's pixels of the squared distance to the nearest feature pixel, comes from the two-pass transform
// of elementwise.hip cut down to the job's crop:
//   columns  one work-item per column of the feature object's column range sweeps the UNION of the two objects' row ranges
//            down and up with the feature test label == f and writes the squared vertical distances of the QUERY's rows only:
//            the job's g2 is query rows x feature columns of scratch
//   rows     one workgroup per query row with that row of g2 in LDS; a work-item runs the outward search of edt_rows_kernel
//            from every pixel of the row with label == q (which may lie outside the feature's columns: the search then starts
//            at the nearest of them), the maxima are reduced per wave and per workgroup and leave as ONE atomicMax per
//            workgroup into out[job's slot]
// Jobs come as a device table of PH_JOB int32 each (medt_abi.h) whose `first block' columns are the prefix sums of the
// blocks the jobs before it take in either launch: a workgroup finds its job by binary search over them.  A job whose
// fields do not fit the images, the scratch or `out' is skipped by both kernels (a check per workgroup, on scalars): the
// table is device memory the host side of this call cannot read.  Integers throughout, integer max: the same bits on every
// run; nobody waits on another workgroup.
constexpr int PH_JOB = MEDT_PAIR_JOB_INTS;
constexpr int PH_FAR = 1 << 30;               // what the row pass holds in LDS for MEDT_EDT_NONE: PH_FAR + 4095^2 < 2^31
enum { PH_N, PH_QLAB, PH_FLAB, PH_SWAP, PH_QY0, PH_QY1, PH_QX0, PH_QX1, PH_FX0, PH_FX1, PH_SY0, PH_SY1, PH_OFF, PH_OUT, PH_COLB, PH_ROWB };

struct PairJob {
    int n, qlab, flab, swap, qy0, qy1, qx0, qx1, fx0, fx1, sy0, sy1, off, out, first;
    bool ok;
};

// the last job whose first block is <= blk (the prefix is non-decreasing and starts at 0), and its fields
__device__ __forceinline__ PairJob pair_job(const int32_t* __restrict__ jobs, int n_jobs, int which, int blk, int N, int H, int W,
                                            long long scratch_elems, int n_out) {
    int lo = 0, hi = n_jobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[(size_t)mid * PH_JOB + which] <= blk) lo = mid; else hi = mid - 1;
    }
    const int32_t* j = jobs + (size_t)lo * PH_JOB;
    PairJob r;
    r.n = j[PH_N]; r.qlab = j[PH_QLAB]; r.flab = j[PH_FLAB]; r.swap = j[PH_SWAP];
    r.qy0 = j[PH_QY0]; r.qy1 = j[PH_QY1]; r.qx0 = j[PH_QX0]; r.qx1 = j[PH_QX1];
    r.fx0 = j[PH_FX0]; r.fx1 = j[PH_FX1]; r.sy0 = j[PH_SY0]; r.sy1 = j[PH_SY1];
    r.off = j[PH_OFF]; r.out = j[PH_OUT]; r.first = j[which];
    r.ok = r.n >= 0 && r.n < N && r.qlab >= 1 && r.flab >= 1 && r.qy0 >= 0 && r.qy0 <= r.qy1 && r.qy1 < H && r.qx0 >= 0 &&
           r.qx0 <= r.qx1 && r.qx1 < W && r.fx0 >= 0 && r.fx0 <= r.fx1 && r.fx1 < W && r.sy0 >= 0 && r.sy0 <= r.qy0 &&
           r.qy1 <= r.sy1 && r.sy1 < H && r.off >= 0 && r.out >= 0 && r.out < n_out && r.first <= blk &&
           (long long)r.off + (long long)(r.qy1 - r.qy0 + 1) * (r.fx1 - r.fx0 + 1) <= scratch_elems;
    return r;
}

__global__ __launch_bounds__(MEDT_THREADS) void pair_cols_kernel(const int32_t* __restrict__ la, const int32_t* __restrict__ lb,
                                                                 const int32_t* __restrict__ jobs, int32_t* __restrict__ scratch,
                                                                 int n_jobs, int N, int H, int W, long long scratch_elems, int n_out) {
    const PairJob j = pair_job(jobs, n_jobs, PH_COLB, (int)blockIdx.x, N, H, W, scratch_elems, n_out);
    if (!j.ok) return;
    const int fw = j.fx1 - j.fx0 + 1;
    const int c = ((int)blockIdx.x - j.first) * MEDT_THREADS + (int)threadIdx.x;         // column of the crop
    if (c >= fw) return;
    const int32_t* f = (j.swap ? la : lb) + (size_t)j.n * H * W + (j.fx0 + c);
    int32_t* g = scratch + (size_t)j.off + c;
    int dist = MEDT_EDT_NONE;
    for (int y = j.sy0; y <= j.sy1; ++y) {                     // down: the nearest feature pixel at or above
        dist = f[(size_t)y * W] == j.flab ? 0 : (dist == MEDT_EDT_NONE ? MEDT_EDT_NONE : dist + 1);
        if (y >= j.qy0 && y <= j.qy1) g[(size_t)(y - j.qy0) * fw] = dist;
    }
    dist = MEDT_EDT_NONE;
    for (int y = j.sy1; y >= j.sy0; --y) {                     // up: the one below, the smaller of the two squared
        if (y >= j.qy0 && y <= j.qy1) {
            int32_t* p = g + (size_t)(y - j.qy0) * fw;
            const int a = *p;
            dist = a == 0 ? 0 : (dist == MEDT_EDT_NONE ? MEDT_EDT_NONE : dist + 1);
            const int d = min(a, dist);
            *p = d == MEDT_EDT_NONE ? MEDT_EDT_NONE : d * d;
        } else {
            dist = f[(size_t)y * W] == j.flab ? 0 : (dist == MEDT_EDT_NONE ? MEDT_EDT_NONE : dist + 1);
        }
    }
}

__global__ __launch_bounds__(MEDT_THREADS) void pair_rows_kernel(const int32_t* __restrict__ la, const int32_t* __restrict__ lb,
                                                                 const int32_t* __restrict__ jobs, const int32_t* __restrict__ scratch,
                                                                 int32_t* __restrict__ out, int n_jobs, int N, int H, int W,
                                                                 long long scratch_elems, int n_out) {
    MEDT_STATIC_SHARED int gs[MEDT_LABEL_MAX_DIM];
    MEDT_STATIC_SHARED int red[MEDT_THREADS / 64];
    const PairJob j = pair_job(jobs, n_jobs, PH_ROWB, (int)blockIdx.x, N, H, W, scratch_elems, n_out);
    if (!j.ok) return;                                         // (uniform over the workgroup: nobody is left at a barrier)
    const int r = (int)blockIdx.x - j.first;
    if (r > j.qy1 - j.qy0) return;
    const int fw = j.fx1 - j.fx0 + 1, y = j.qy0 + r, tid = threadIdx.x;
    const int32_t* g = scratch + (size_t)j.off + (size_t)r * fw;
    for (int i = tid; i < fw; i += MEDT_THREADS) gs[i] = min(g[i], PH_FAR);
    __syncthreads();
    const int32_t* q = (j.swap ? lb : la) + ((size_t)j.n * H + y) * W;
    int worst = 0;
    for (int x = j.qx0 + tid; x <= j.qx1; x += MEDT_THREADS) {
        if (q[x] != j.qlab) continue;
        int best = PH_FAR;
        const int reach = max(x - j.fx0, j.fx1 - x);           // the farthest feature column
        for (int d = max(0, max(j.fx0 - x, x - j.fx1)); d <= reach; ++d) {     // from the nearest one outwards, both sides at once
            const int dd = d * d;
            if (dd >= best) break;
            const int xl = x - d, xr = x + d;
            if (xl >= j.fx0 && xl <= j.fx1) best = min(best, gs[xl - j.fx0] + dd);
            if (xr >= j.fx0 && xr <= j.fx1) best = min(best, gs[xr - j.fx0] + dd);
        }
        if (best >= PH_FAR) best = MEDT_EDT_NONE;              // a feature object without a pixel (the host refuses such a pair)
        worst = max(worst, best);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) worst = max(worst, __shfl_xor(worst, o, 64));
    if ((tid & 63) == 0) red[tid >> 6] = worst;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < MEDT_THREADS / 64; ++w) worst = max(worst, red[w]);
        if (worst > 0) atomicMax(out + j.out, worst);          // (out starts at 0 and distances are >= 0)
    }
}

int pair_hausdorff(const int32_t* la, const int32_t* lb, const int32_t* jobs, int32_t* scratch, int32_t* out, int n_jobs,
                   int col_blocks, int row_blocks, size_t scratch_elems, int n_out, int clear_out, int N, int H, int W, hipStream_t s) {
    if (clear_out && hipMemsetAsync(out, 0, (size_t)n_out * sizeof(int32_t), s) != hipSuccess) {
        set_error("pair_hausdorff: clearing out failed"); return MEDT_ELAUNCH;
    }
    const dim3 block(MEDT_THREADS);
    hipLaunchKernelGGL(pair_cols_kernel, dim3((unsigned)col_blocks), block, 0, s, la, lb, jobs, scratch, n_jobs, N, H, W,
                       (long long)scratch_elems, n_out);
    hipLaunchKernelGGL(pair_rows_kernel, dim3((unsigned)row_blocks), block, 0, s, la, lb, jobs, scratch, out, n_jobs, N, H, W,
                       (long long)scratch_elems, n_out);
    return launch_status("pair_hausdorff");
}

}  // namespace medt
