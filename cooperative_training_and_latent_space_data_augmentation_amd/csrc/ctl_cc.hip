// Connected components of label volumes on device (include/ctl_hip.h, "connected components"):
//   ctl_cc_label          canonical component labels of every foreground class
//   ctl_cc_keep_largest   medseg/common_utils/post_process.py:5-22 (keep_largest_connected_components) without the host round trip
//
// A component is a maximal connected set of voxels of ONE class c, 1 <= c < n_class; its label is the smallest C-order linear index of
// its voxels (within the volume in the 3-D form, within the slice in the 2-D form).  The labels live in a parent array P (int32 per
// voxel, -1 = no class) that is a union-find forest with ONE invariant: P[x] <= x.  A root is a voxel with P[x] == x, so the root of a
// finished tree IS the canonical label, whatever the order of the merges was.  The launches of one call, whatever the volume holds:
//   1. cc_tile_kernel     union-find of every 16 x 64 tile of a slice in LDS (rows as runs, then the vertical / diagonal links);
//                         P = the tile's own roots, size = voxels per tile root (counted in LDS, one add per run)
//   2. cc_merge_kernel    links that cross a tile border and, in the 3-D form, a slice boundary: atomicMin on P in global memory
//   3. cc_flatten_kernel  P[x] = root of x; the size of every tile root is added to its final root: ONE atomic per (tile, component)
//   4. cc_select_kernel   per (group, class): atomicMax of (size << 32) | (0xFFFFFFFF - label) over the roots (largest, then first in C
//                         order), and the number of roots; both reduced per block in LDS first
//   5. cc_output_kernel   out = class where P == the selected label, else 0; the table
// i.e. 3 launches for ctl_cc_label (1-3, P = the caller's label array) and 5 for ctl_cc_keep_largest.  Integer atomics only (min, max,
// add): every result is independent of arrival order, the same bits on every call.
#include "ctl_device.h"

#define CC_THREADS 256
#define CC_TW 64                       // tile width: the lanes of a wave
#define CC_TH 16                       // tile height: 4 rows per wave
#define CC_RPT (CC_TH / (CC_THREADS / 64))

__device__ __forceinline__ int cc_class(uint8_t v, int n) { return v < n ? (int)v : 0; }

// P is read and written by many threads at once (LDS in kernel 1, global memory in kernels 2 and 3): relaxed atomic accesses, so a
// value is never kept in a register across a retry and a global read is served by L2, where the atomicMin of another CU landed.
__device__ __forceinline__ int cc_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Terminates: P[x] <= x always (the only writes are atomicMin with a smaller value and the flattening store of an ancestor), so x
// strictly decreases until a root.
__device__ __forceinline__ int cc_find(const int* P, int x) {
    int p;
    while ((p = cc_ld(P + x)) != x) x = p;
    return x;
}

// Union by smaller index.  a > b are roots as far as this thread saw; atomicMin(P[a], b) returns a iff a still was a root, and then a's
// tree hangs below b: done.  Otherwise somebody linked a first (old < a): P[a] is now min(old, b), either way a stays in a set with old
// or with b, and what is left to do is union(old, b).  Terminates for every input: a failed attempt replaces a by old < a, find never
// increases a or b, and both are >= 0, so after finitely many failures the attempt succeeds or a == b.
__device__ __forceinline__ void cc_union(int* P, int a, int b) {
    a = cc_find(P, a);
    b = cc_find(P, b);
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(P + a, b);
        if (old == a) break;
        a = cc_find(P, old);
        b = cc_find(P, b);
    }
}

// ------------------------------------------------------------------------------------------------ 1. tiles
// blockIdx.x = (z * tiles_y + ty) * tiles_x + tx.  voff: what a stored label adds to the in-slice index (z * H * W in the 3-D form, 0 in
// the 2-D form).  In-tile order y * 64 + x is C order, so the smallest in-tile index is the smallest global index of the tile's part.
// conn2 = in-slice connectivity (1: 4-neighbourhood, 2: 8-neighbourhood).  A diagonal link is only needed when neither of the two
// voxels that complete the square carries the class (otherwise the two are linked through it).
__global__ __launch_bounds__(CC_THREADS) void cc_tile_kernel(const uint8_t* __restrict__ lab, int H, int W, int n, int mode, int conn2,
                                                             int tiles_x, int tiles_y, int32_t* __restrict__ P, int32_t* __restrict__ size,
                                                             unsigned long long* __restrict__ best, int32_t* __restrict__ ncomp, int nsel) {
    __shared__ int par[CC_TH * CC_TW];
    __shared__ int cnt[CC_TH * CC_TW];
    __shared__ uint8_t cls[CC_TH][CC_TW];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y, z = blockIdx.x / (tiles_x * tiles_y);
    const int plane = H * W, zbase = z * plane, voff = mode == 3 ? zbase : 0;
    const int gx = tx * CC_TW + lane;
    if (best && blockIdx.x == 0)                                               // the selection cells of kernel 4 start from zero
        for (int i = threadIdx.x; i < nsel; i += CC_THREADS) { best[i] = 0ull; ncomp[i] = 0; }
    int runlen[CC_RPT];                                                        // > 0: this lane starts a run of its class, of that many voxels
#pragma unroll
    for (int k = 0; k < CC_RPT; ++k) {
        const int r = w + k * (CC_THREADS / 64), gy = ty * CC_TH + r;
        const int c = (gy < H && gx < W) ? cc_class(lab[zbase + gy * W + gx], n) : 0;
        const int cl = __shfl_up(c, 1);
        const bool bnd = lane == 0 || cl != c;
        int s = bnd ? lane : 0;                                                // max-scan: the start of the run this lane is in
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(s, d);
            if (lane >= d) s = max(s, t);
        }
        const unsigned long long mask = __ballot(bnd);
        const unsigned long long higher = lane == 63 ? 0ull : mask >> (lane + 1);
        const int len = higher ? __ffsll(higher) : 64 - lane;
        runlen[k] = (bnd && c) ? len : 0;
        par[r * CC_TW + lane] = r * CC_TW + s;
        cnt[r * CC_TW + lane] = 0;
        cls[r][lane] = (uint8_t)c;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CC_RPT; ++k) {
        const int r = w + k * (CC_THREADS / 64), i = r * CC_TW + lane;
        const int c = cls[r][lane];
        if (r == 0 || c == 0) continue;
        const int up = cls[r - 1][lane];
        const int left = lane > 0 ? cls[r][lane - 1] : 0, ul = lane > 0 ? cls[r - 1][lane - 1] : 0;
        if (up == c) {
            if (!(left == c && ul == c)) cc_union(par, i, i - CC_TW);          // else the lane to the left makes the same link
        } else if (conn2 == 2) {
            if (ul == c && left != c) cc_union(par, i, i - CC_TW - 1);
            if (lane < 63 && cls[r - 1][lane + 1] == c && cls[r][lane + 1] != c) cc_union(par, i, i - CC_TW + 1);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CC_RPT; ++k) {
        const int r = w + k * (CC_THREADS / 64);
        if (runlen[k]) atomicAdd(&cnt[cc_find(par, r * CC_TW + lane)], runlen[k]);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CC_RPT; ++k) {
        const int r = w + k * (CC_THREADS / 64), i = r * CC_TW + lane, gy = ty * CC_TH + r;
        if (gy >= H || gx >= W) continue;
        const int c = cls[r][lane];
        const int root = c ? cc_find(par, i) : -1;
        const int a = zbase + gy * W + gx;
        P[a] = c ? voff + (ty * CC_TH + root / CC_TW) * W + tx * CC_TW + root % CC_TW : -1;
        if (size) size[a] = root == i ? cnt[i] : 0;
    }
}

// ------------------------------------------------------------------------------------------------ 2. borders
// One thread per voxel; it makes the links to its PRECEDING neighbours (left, the row above, the slice below it in memory) that kernel 1
// could not see.  A link is skipped when the voxel to the left makes an equivalent one: that voxel is in the same tile and row, so the
// two are already in one set, and so are their two partners.  conn = the caller's connectivity: in the 3-D form the neighbours of the
// previous slice are those at in-plane L1 offset <= conn - 1.
__global__ __launch_bounds__(CC_THREADS) void cc_merge_kernel(const uint8_t* __restrict__ lab, int D, int H, int W, int n, int mode, int conn,
                                                              int32_t* P) {
    const int plane = H * W;
    const int64_t a64 = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (a64 >= (int64_t)D * plane) return;
    const int a = (int)a64;
    const int c = cc_class(lab[a], n);
    if (!c) return;
    const int z = a / plane, s = a - z * plane, y = s / W, x = s - y * W;
    const int ly = y % CC_TH, lx = x % CC_TW;
    const uint8_t* sl = lab + (a - s);
    int32_t* Ps = mode == 2 ? P + (a - s) : P;                                 // labels index Ps directly
    const int v = mode == 2 ? s : a;
    const int conn2 = conn < 2 ? conn : 2;
    const int up = y > 0 ? cc_class(sl[s - W], n) : 0, left = x > 0 ? cc_class(sl[s - 1], n) : 0;
    const int ul = (y > 0 && x > 0) ? cc_class(sl[s - W - 1], n) : 0;
    if (lx == 0 && left == c && !(ly > 0 && up == c && ul == c)) cc_union(Ps, v, v - 1);
    if (ly == 0 && up == c && !(lx > 0 && left == c && ul == c)) cc_union(Ps, v, v - W);
    if (conn2 == 2 && y > 0 && up != c) {
        if ((ly == 0 || lx == 0) && ul == c && left != c) cc_union(Ps, v, v - W - 1);
        if ((ly == 0 || lx == CC_TW - 1) && x + 1 < W && cc_class(sl[s - W + 1], n) == c && cc_class(sl[s + 1], n) != c)
            cc_union(Ps, v, v - W + 1);
    }
    if (mode == 3 && z > 0) {
        const uint8_t* dn = sl - plane;
        if (cc_class(dn[s], n) == c) {
            if (!(lx > 0 && left == c && cc_class(dn[s - 1], n) == c)) cc_union(P, a, a - plane);
        } else if (conn >= 2) {
            // (dy, dx) != (0, 0): needed only if neither dn[s] (checked above) nor the voxel of THIS slice at the offset carries the class
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int l1 = abs(dy) + abs(dx);
                    const int yy = y + dy, xx = x + dx;
                    if (l1 == 0 || l1 > conn - 1 || yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
                    const int o = dy * W + dx;
                    if (cc_class(dn[s + o], n) == c && cc_class(sl[s + o], n) != c) cc_union(P, a, a - plane + o);
                }
        }
    }
}

// ------------------------------------------------------------------------------------------------ 3. flatten, sizes
// Nothing links any more, so find(x) is the final root for every thread; storing it into P[x] while others still walk through x only
// shortens their way (it is an ancestor of x and <= the old value).
__global__ __launch_bounds__(CC_THREADS) void cc_flatten_kernel(int D, int plane, int mode, int32_t* P, int32_t* size) {
    const int64_t a64 = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (a64 >= (int64_t)D * plane) return;
    const int a = (int)a64;
    if (cc_ld(P + a) < 0) return;
    const int base = mode == 2 ? (a / plane) * plane : 0;
    const int v = a - base;
    const int r = cc_find(P + base, v);
    __hip_atomic_store(P + a, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (size) {
        const int sz = size[a];                                                // > 0: a tile root; only a final root (r == v) receives adds
        if (sz > 0 && r != v) atomicAdd(size + base + r, sz);
    }
}

// ------------------------------------------------------------------------------------------------ 4. selection
// blockIdx.x = group * bpg + chunk: a block never straddles two groups (slices in the 2-D form), so one LDS cell per class reduces the
// block's roots before ONE global atomic per (block, class that has a root here).
__global__ __launch_bounds__(CC_THREADS) void cc_select_kernel(const uint8_t* __restrict__ lab, const int32_t* __restrict__ P,
                                                               const int32_t* __restrict__ size, int per, int bpg, int n,
                                                               unsigned long long* __restrict__ best, int32_t* __restrict__ ncomp) {
    __shared__ unsigned long long sbest[256];
    __shared__ int scount[256];
    const int g = blockIdx.x / bpg, v = (blockIdx.x % bpg) * CC_THREADS + threadIdx.x;
    sbest[threadIdx.x] = 0ull;
    scount[threadIdx.x] = 0;
    __syncthreads();
    if (v < per) {
        const int64_t a = (int64_t)g * per + v;
        if (P[a] == v) {
            const int c = cc_class(lab[a], n);
            atomicMax(&sbest[c - 1], ((unsigned long long)(unsigned)size[a] << 32) | (0xFFFFFFFFu - (unsigned)v));
            atomicAdd(&scount[c - 1], 1);
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < n - 1 && scount[threadIdx.x]) {
        atomicMax(&best[(int64_t)g * (n - 1) + threadIdx.x], sbest[threadIdx.x]);
        atomicAdd(&ncomp[(int64_t)g * (n - 1) + threadIdx.x], scount[threadIdx.x]);
    }
}

// ------------------------------------------------------------------------------------------------ 5. output
// lab and out may be the same array: a thread reads its own voxel before it writes it.
__global__ __launch_bounds__(CC_THREADS) void cc_output_kernel(const uint8_t* lab, const int32_t* __restrict__ P, int per, int bpg, int n,
                                                               const unsigned long long* __restrict__ best,
                                                               const int32_t* __restrict__ ncomp, int nsel, uint8_t* out,
                                                               int64_t* __restrict__ table) {
    const int g = blockIdx.x / bpg, v = (blockIdx.x % bpg) * CC_THREADS + threadIdx.x;
    if (table && blockIdx.x == 0)
        for (int i = threadIdx.x; i < nsel; i += CC_THREADS) {
            const unsigned long long b = best[i];
            const int k = ncomp[i];
            table[3 * i + 0] = k;
            table[3 * i + 1] = k ? (int64_t)(b >> 32) : 0;
            table[3 * i + 2] = k ? (int64_t)(0xFFFFFFFFu - (unsigned)(b & 0xFFFFFFFFull)) : -1;
        }
    if (v >= per) return;
    const int64_t a = (int64_t)g * per + v;
    const int c = cc_class(lab[a], n);
    uint8_t o = 0;
    if (c) {
        const unsigned keep = 0xFFFFFFFFu - (unsigned)(best[(int64_t)g * (n - 1) + c - 1] & 0xFFFFFFFFull);
        o = (unsigned)P[a] == keep ? (uint8_t)c : (uint8_t)0;
    }
    out[a] = o;
}

// ------------------------------------------------------------------------------------------------ host side
struct cc_plan {
    int64_t vox, groups, nsel;         // voxels, groups (slices in the 2-D form, else 1), selection cells = groups * (n_class - 1)
    int per, bpg;                      // voxels per group, blocks per group of kernels 4 and 5
    int tiles_x, tiles_y;
    size_t off_parent, off_size, off_best, off_ncomp, bytes;
};

static int cc_make_plan(const char* who, int32_t d, int32_t h, int32_t w, int32_t n_class, int32_t mode, cc_plan* p) {
    CTL_REQUIRE(d >= 1 && h >= 1 && w >= 1, "%s: D, H, W must be positive (got %d, %d, %d)", who, d, h, w);
    CTL_REQUIRE(n_class >= 2 && n_class <= 255, "%s: n_class %d outside 2..255", who, n_class);
    CTL_REQUIRE(mode == 2 || mode == 3, "%s: mode must be 2 (per-slice 2-D) or 3 (whole-volume 3-D), got %d", who, mode);
    p->vox = (int64_t)d * h * w;
    CTL_REQUIRE((int64_t)h * w < (1ll << 31) && p->vox < (1ll << 31),
                "%s: labels are 32-bit linear indices, a volume of %lld voxels (2^31 or more) is not supported", who, (long long)p->vox);
    p->groups = mode == 2 ? d : 1;
    p->nsel = p->groups * (n_class - 1);
    p->per = (int)(mode == 2 ? (int64_t)h * w : p->vox);
    p->bpg = ctl_cdiv(p->per, CC_THREADS);
    p->tiles_x = ctl_cdiv(w, CC_TW);
    p->tiles_y = ctl_cdiv(h, CC_TH);
    CTL_REQUIRE(p->groups * p->bpg < (1ll << 31) && (int64_t)d * p->tiles_x * p->tiles_y < (1ll << 31) && p->nsel < (1ll << 31),
                "%s: the problem is too large for one launch (%lld voxels)", who, (long long)p->vox);
    size_t off = 0;
    p->off_parent = off; off += ctl_align256((size_t)p->vox * sizeof(int32_t));
    p->off_size = off; off += ctl_align256((size_t)p->vox * sizeof(int32_t));
    p->off_best = off; off += ctl_align256((size_t)p->nsel * sizeof(unsigned long long));
    p->off_ncomp = off; off += ctl_align256((size_t)p->nsel * sizeof(int32_t));
    p->bytes = off;
    return CTL_OK;
}

static int cc_check_conn(const char* who, int32_t mode, int32_t connectivity) {
    CTL_REQUIRE(connectivity >= 1 && connectivity <= mode, "%s: connectivity %d outside 1..%d", who, connectivity, mode);
    return CTL_OK;
}

// kernels 1-3: the forest in P, flattened; size == NULL: labels only
static int cc_label_launches(const cc_plan& p, const uint8_t* labelmap, int32_t d, int32_t h, int32_t w, int32_t n_class, int32_t mode,
                             int32_t connectivity, int32_t* P, int32_t* size, unsigned long long* best, int32_t* ncomp, ctl_stream stream) {
    const int conn2 = connectivity < 2 ? connectivity : 2;
    const unsigned vox_blocks = (unsigned)ctl_cdiv64(p.vox, CC_THREADS);
    cc_tile_kernel<<<dim3((unsigned)((int64_t)d * p.tiles_x * p.tiles_y)), dim3(CC_THREADS), 0, S_>>>(labelmap, h, w, n_class, mode, conn2, p.tiles_x,
                                                                                                    p.tiles_y, P, size, best, ncomp, (int)p.nsel);
    CTL_LAUNCH_CHECK("cc_tiles");
    cc_merge_kernel<<<dim3(vox_blocks), dim3(CC_THREADS), 0, S_>>>(labelmap, d, h, w, n_class, mode, connectivity, P);
    CTL_LAUNCH_CHECK("cc_merge");
    cc_flatten_kernel<<<dim3(vox_blocks), dim3(CC_THREADS), 0, S_>>>(d, h * w, mode, P, size);
    CTL_LAUNCH_CHECK("cc_flatten");
    return CTL_OK;
}

extern "C" size_t ctl_cc_ws_bytes(int32_t d, int32_t h, int32_t w, int32_t n_class, int32_t mode) {
    cc_plan p;
    if (cc_make_plan("cc_ws_bytes", d, h, w, n_class, mode, &p)) return 0;
    return p.bytes;
}

extern "C" int ctl_cc_label(const uint8_t* labelmap, int32_t d, int32_t h, int32_t w, int32_t n_class, int32_t mode, int32_t connectivity,
                            int32_t* labels, ctl_stream stream) {
    cc_plan p;
    int rc = cc_make_plan("cc_label", d, h, w, n_class, mode, &p);
    if (rc || (rc = cc_check_conn("cc_label", mode, connectivity))) return rc;
    CTL_REQUIRE(labelmap && labels, "cc_label: null pointer");
    return cc_label_launches(p, labelmap, d, h, w, n_class, mode, connectivity, labels, nullptr, nullptr, nullptr, stream);
}

extern "C" int ctl_cc_keep_largest(const uint8_t* labelmap, int32_t d, int32_t h, int32_t w, int32_t n_class, int32_t mode,
                                   int32_t connectivity, uint8_t* out, int64_t* table, void* workspace, size_t workspace_bytes,
                                   ctl_stream stream) {
    cc_plan p;
    int rc = cc_make_plan("cc_keep_largest", d, h, w, n_class, mode, &p);
    if (rc || (rc = cc_check_conn("cc_keep_largest", mode, connectivity))) return rc;
    CTL_REQUIRE(labelmap && out && workspace, "cc_keep_largest: null pointer");
    CTL_REQUIRE(workspace_bytes >= p.bytes, "cc_keep_largest: workspace of %zu bytes, %zu needed", workspace_bytes, p.bytes);
    char* ws = (char*)workspace;
    int32_t* P = (int32_t*)(ws + p.off_parent);
    int32_t* size = (int32_t*)(ws + p.off_size);
    unsigned long long* best = (unsigned long long*)(ws + p.off_best);
    int32_t* ncomp = (int32_t*)(ws + p.off_ncomp);
    if ((rc = cc_label_launches(p, labelmap, d, h, w, n_class, mode, connectivity, P, size, best, ncomp, stream))) return rc;
    const dim3 grid((unsigned)(p.groups * p.bpg));
    cc_select_kernel<<<grid, dim3(CC_THREADS), 0, S_>>>(labelmap, P, size, p.per, p.bpg, n_class, best, ncomp);
    CTL_LAUNCH_CHECK("cc_select");
    cc_output_kernel<<<grid, dim3(CC_THREADS), 0, S_>>>(labelmap, P, p.per, p.bpg, n_class, best, ncomp, (int)p.nsel, out, table);
    CTL_LAUNCH_CHECK("cc_output");
    return CTL_OK;
}
