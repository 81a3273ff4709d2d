// dcte_vmap.hip -- the seam visibility map of a carve loop and what liblqr
// answers from it (include/dctenergy.h, "seam visibility map"): resizing to
// any width within the carved depth, enlarging, and the "Seams" layer.
//
//   dcte_vmap_row / dcte_vmap_wide   per-step seam columns -> visibility map
//   dcte_vmap_render                 frame + map + delta   -> resized frame
//   dcte_vmap_seams_u8               frame + map           -> seams overlay
//
// Rows are independent everywhere; inside a row the steps of the map are
// sequential (step k removes the c-th pixel still alive), the render is a
// stream compaction / expansion with a running output offset.
//
// The two conventions taken from liblqr without a liblqr to check them
// against [liblqr, unverified] live in one function each, so that pinning
// one later is a one-line change: vmap_level (which number a step writes)
// and vmap_inserted (the value of a pixel inserted when enlarging).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dcte_kernels.h"

namespace dcte {

// the number step k (0-based) leaves at the pixel it removes [liblqr, unverified]
__device__ __forceinline__ int vmap_level(int k) { return k + 1; }

// one channel of the pixel inserted left of pixel x when enlarging: the
// integer mean of the pixel and its left neighbour (x = 0: the pixel itself),
// truncated [liblqr, unverified]
__device__ __forceinline__ unsigned vmap_inserted(unsigned left, unsigned here)
{
    return (left + here) >> 1;
}

// green of a seam pixel of the "Seams" layer: 255 * vis / depth in double,
// truncated (src/render.c:228-230)
__device__ __forceinline__ uint8_t vmap_green(int vis, int depth)
{
    return depth > 0 ? (uint8_t)(long long)(255.0 * (double)vis / (double)depth) : (uint8_t)255;
}

__device__ __forceinline__ unsigned long long lanes_below(int lane)
{
    return (1ull << lane) - 1ull;
}

// position of the n-th (0-based) set bit of m; n < popcount(m), anything
// (in [0, 63]) otherwise
__device__ __forceinline__ int select64(unsigned long long m, int n)
{
    unsigned w = (unsigned)m;
    int pos = 0;
    int pc = __popc(w);
    if (n >= pc) {
        n -= pc;
        pos = 32;
        w = (unsigned)(m >> 32);
    }
#pragma unroll
    for (int s = 16; s >= 1; s >>= 1) {
        pc = __popc(w & ((1u << s) - 1u));
        if (n >= pc) {
            n -= pc;
            pos += s;
            w >>= s;
        }
    }
    return pos;
}

__device__ __forceinline__ int wave_scan_incl(int v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

// ---- visibility map, rows of at most 64 * 64 * WPL pixels: one wave per row.
// Lane l keeps the alive bits of pixels [64 WPL l, 64 WPL (l + 1)) in WPL
// 64-bit registers, their number, and the inclusive prefix of those numbers
// over the lanes.  A step: the owning lane is the first whose prefix exceeds
// c (one ballot); it selects the (c - its exclusive prefix)-th set bit of its
// words, writes the level there and clears the bit; every lane from the owner
// on lowers its prefix by one.  The step columns arrive 64 at a time (lane j
// loads step k0 + j).  The pixels still alive at the end are written 0
// afterwards, word by word (coalesced), so every entry is stored exactly once.
template <int WPL>
__global__ __launch_bounds__(256) void dcte_vmap_row(const VmapParams p)
{
    const int y = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (y >= p.h) return;
    const int W = p.w;
    int32_t* row = p.vmap + (long long)y * p.stride;
    unsigned long long m[WPL];
    int cnt = 0;
#pragma unroll
    for (int i = 0; i < WPL; i++) {
        const int x0 = (lane * WPL + i) * 64;
        const int nb = W - x0;                       // valid bits of this word
        m[i] = nb >= 64 ? ~0ull : nb > 0 ? (1ull << nb) - 1ull : 0ull;
        cnt += __popcll(m[i]);
    }
    int incl = wave_scan_incl(cnt, lane);
    int cvals = 0;
    for (int k = 0; k < p.depth; k++) {
        if ((k & 63) == 0) {
            const int kk = k + lane;
            cvals = kk < p.depth ? p.seams[(long long)kk * p.h + y] : 0;
        }
        const int len = W - k;                       // pixels alive (depth < W: len >= 1)
        int c = __builtin_amdgcn_readlane(cvals, k & 63);
        c = c < 0 ? 0 : c > len - 1 ? len - 1 : c;   // dcte_seam_carve_device's clamp
        const unsigned long long above = __ballot(incl > c);
        if (above == 0) break;                       // (incl[63] = len > c: never)
        const int owner = __ffsll((long long)above) - 1;
        int n = c - (incl - cnt);                    // in the owner: rank inside its words
        int wi = 0;
        unsigned long long mw = m[0];
#pragma unroll
        for (int i = 0; i + 1 < WPL; i++) {
            const int pc = __popcll(m[i]);
            if (wi == i && n >= pc) {
                n -= pc;
                wi = i + 1;
                mw = m[i + 1];
            }
        }
        const int bit = select64(mw, n);
        if (lane == owner) {
            const int x = (lane * WPL + wi) * 64 + bit;
            if (x < W) row[x] = vmap_level(k);
#pragma unroll
            for (int i = 0; i < WPL; i++)
                if (wi == i) m[i] &= ~(1ull << bit);
            cnt--;
        }
        if (lane >= owner) incl--;
    }
#pragma unroll
    for (int i = 0; i < WPL; i++) {
        for (int l = 0; l < 64; l++) {
            const int x0 = (l * WPL + i) * 64;
            if (x0 >= W) break;
            const unsigned lo = __builtin_amdgcn_readlane((unsigned)m[i], l);
            const unsigned hi = __builtin_amdgcn_readlane((unsigned)(m[i] >> 32), l);
            const unsigned long long word = ((unsigned long long)hi << 32) | lo;
            if ((word >> lane) & 1ull) row[x0 + lane] = 0;
        }
    }
}

// ---- visibility map, any width: one wave per row.  The row of the map is
// its own alive mask (0 = alive); the wave keeps in LDS the alive count of
// each of <= 4096 blocks of `blk` consecutive pixels, and in registers the
// counts of the 64 super-blocks of 64 blocks with their inclusive prefix.  A
// step: ballot over the super-block prefix, a wave scan of that super-block's
// 64 block counts, then a walk over the block's pixels 64 at a time (ballot
// of "still 0", popcount, select).  The wave reads map entries it stored in
// earlier steps: the workgroup barrier after each step orders them.
constexpr int kWideBlocks = 4096;

__global__ __launch_bounds__(64) void dcte_vmap_wide(const VmapParams p)
{
    __shared__ int cnt[kWideBlocks];
    const int y = blockIdx.x;
    const int lane = threadIdx.x;
    const long long W = p.w, P = p.blk;
    int32_t* row = p.vmap + (long long)y * p.stride;
    for (long long x = lane; x < W; x += 64) row[x] = 0;
    for (int b = lane; b < kWideBlocks; b += 64) {
        const long long left = W - (long long)b * P;
        cnt[b] = left >= P ? (int)P : left > 0 ? (int)left : 0;
    }
    __syncthreads();
    int sup = 0;                                     // alive in super-block `lane`
    for (int j = 0; j < 64; j++) sup += cnt[lane * 64 + ((j + lane) & 63)];
    int incl = wave_scan_incl(sup, lane);
    int cvals = 0;
    for (int k = 0; k < p.depth; k++) {
        if ((k & 63) == 0) {
            const int kk = k + lane;
            cvals = kk < p.depth ? p.seams[(long long)kk * p.h + y] : 0;
        }
        const int len = (int)W - k;
        int c = __builtin_amdgcn_readlane(cvals, k & 63);
        c = c < 0 ? 0 : c > len - 1 ? len - 1 : c;
        const unsigned long long above = __ballot(incl > c);
        if (above == 0) break;                       // (never: incl[63] = len > c)
        const int sb = __ffsll((long long)above) - 1;
        int n = c - (__builtin_amdgcn_readlane(incl, sb) - __builtin_amdgcn_readlane(sup, sb));
        const int bc = cnt[sb * 64 + lane];
        const int binc = wave_scan_incl(bc, lane);
        const unsigned long long babove = __ballot(binc > n);
        if (babove == 0) break;                      // (never: the super-block holds > n)
        const int bl = __ffsll((long long)babove) - 1;
        n -= __builtin_amdgcn_readlane(binc, bl) - __builtin_amdgcn_readlane(bc, bl);
        const int b = sb * 64 + bl;
        const long long base = (long long)b * P;
        const long long end = base + P < W ? base + P : W;
        long long x = -1;
        for (long long q = base; q < end; q += 64) {
            const long long xx = q + lane;
            const int v = xx < end ? row[xx] : 1;
            const unsigned long long alive = __ballot(v == 0);
            const int pc = __popcll(alive);
            if (n < pc) {
                x = q + select64(alive, n);
                break;
            }
            n -= pc;
        }
        if (x < 0) break;                            // (never: the block holds > n)
        if (lane == 0) {
            row[x] = vmap_level(k);
            cnt[b]--;
        }
        if (lane == sb) sup--;
        if (lane >= sb) incl--;
        __syncthreads();
    }
}

// ---- render: one wave per row, 64 pixels per pass.  Pixel x emits 0, 1 or
// 2 output pixels (shrinking: itself unless removed within the first -delta
// steps; enlarging: an inserted pixel first when it was removed within the
// first delta steps); its output position is the row's running offset plus
// the ballot/popcount prefix of the emits of the lanes below it.
template <int BPP, bool DWORD>
__device__ __forceinline__ void load_px(const uint8_t* p, unsigned (&v)[4])
{
    if constexpr (DWORD) {
        const uint32_t u = *reinterpret_cast<const uint32_t*>(p);
        v[0] = u & 255u;
        v[1] = (u >> 8) & 255u;
        v[2] = (u >> 16) & 255u;
        v[3] = u >> 24;
    } else {
#pragma unroll
        for (int c = 0; c < BPP; c++) v[c] = p[c];
    }
}

template <int BPP, bool DWORD>
__device__ __forceinline__ void store_px(uint8_t* p, const unsigned (&v)[4])
{
    if constexpr (DWORD) {
        *reinterpret_cast<uint32_t*>(p) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
    } else {
#pragma unroll
        for (int c = 0; c < BPP; c++) p[c] = (uint8_t)v[c];
    }
}

constexpr int kRenderPasses = 4;

// DWORD (BPP 4, both frames 4-byte aligned with 4-byte-multiple row strides):
// a pixel moves as one dword
template <int BPP, bool DWORD>
__global__ __launch_bounds__(256) void dcte_vmap_render(const RenderParams p)
{
    const int y = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (y >= p.h) return;
    const int W = p.w, Wo = p.w + p.delta;
    // (source and destination never overlap: dcte_vmap_render_device refuses it)
    const uint8_t* __restrict__ src = p.px + (long long)y * p.rowstride;
    const int32_t* __restrict__ vrow = p.vmap + (long long)y * p.vmap_stride;
    uint8_t* __restrict__ dst = p.out + (long long)y * p.out_rowstride;
    const unsigned long long below = lanes_below(lane);
    int off = 0;
    // kRenderPasses passes per trip, loads before stores: a wave walks its row
    // alone, so what it has in flight is what hides the latency
    for (int x0 = 0; x0 < W; x0 += 64 * kRenderPasses) {
        int v[kRenderPasses], pos[kRenderPasses];
        bool keep[kRenderPasses], ins[kRenderPasses];
        unsigned here[kRenderPasses][4], left[kRenderPasses][4];
#pragma unroll
        for (int j = 0; j < kRenderPasses; j++) {
            const int x = x0 + 64 * j + lane;
            v[j] = x < W ? vrow[x] : 0;
        }
#pragma unroll
        for (int j = 0; j < kRenderPasses; j++) {
            const bool in = x0 + 64 * j + lane < W;
            if (p.delta <= 0) {
                keep[j] = in && (v[j] == 0 || v[j] > -p.delta);
                ins[j] = false;
            } else {
                keep[j] = in;
                ins[j] = in && v[j] > 0 && v[j] <= p.delta;
            }
            const unsigned long long bk = __ballot(keep[j]), bi = __ballot(ins[j]);
            pos[j] = off + __popcll(bk & below) + __popcll(bi & below);
            off += __popcll(bk) + __popcll(bi);
        }
#pragma unroll
        for (int j = 0; j < kRenderPasses; j++) {
            const int x = x0 + 64 * j + lane;
#pragma unroll
            for (int c = 0; c < 4; c++) here[j][c] = left[j][c] = 0u;
            if (keep[j]) load_px<BPP, DWORD>(src + (long long)x * BPP, here[j]);
            if (ins[j]) load_px<BPP, DWORD>(src + (long long)(x > 0 ? x - 1 : 0) * BPP, left[j]);
        }
#pragma unroll
        for (int j = 0; j < kRenderPasses; j++) {
            int q = pos[j];
            if (ins[j]) {
                unsigned mid[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                for (int c = 0; c < BPP; c++) mid[c] = vmap_inserted(left[j][c], here[j][c]);
                if (q < Wo) store_px<BPP, DWORD>(dst + (long long)q * BPP, mid);
                q++;
            }
            if (keep[j] && q < Wo) store_px<BPP, DWORD>(dst + (long long)q * BPP, here[j]);
        }
    }
}

// ---- "Seams" layer: a copy of the frame with every removed pixel painted
// (0, G, 0), G = vmap_green; the last row and the last column are never
// painted (the reference's loop bounds, src/render.c:222-223); alpha stays.
// bpp 1: the grey byte becomes G (a deviation: the reference's 3-byte pixel
// on a grey drawable degenerates to 0).  One workgroup per row.
template <int BPP>
__global__ __launch_bounds__(256) void dcte_vmap_seams_u8(const RenderParams p)
{
    const int y = blockIdx.x;
    const uint8_t* src = p.px + (long long)y * p.rowstride;
    const int32_t* vrow = p.vmap + (long long)y * p.vmap_stride;
    uint8_t* dst = p.out + (long long)y * p.out_rowstride;
    for (int x = threadIdx.x; x < p.w; x += 256) {
        unsigned px[4] = {0u, 0u, 0u, 0u};
        load_px<BPP, false>(src + (long long)x * BPP, px);
        const int vis = vrow[x];
        if (vis != 0 && x < p.w - 1 && y < p.h - 1) {
            const unsigned g = vmap_green(vis, p.depth);
            if constexpr (BPP == 1) {
                px[0] = g;
            } else {
                px[0] = 0u;
                px[1] = g;
                px[2] = 0u;
            }
        }
        store_px<BPP, false>(dst + (long long)x * BPP, px);
    }
}

// ------------------------------------------------------------------ launchers
int vmap_wave_max_w(int words_per_lane) { return 64 * 64 * words_per_lane; }

hipError_t launch_vmap(const VmapParams& q, hipStream_t s)
{
    if (q.w < 1 || q.h < 1 || q.depth < 0 || q.depth >= q.w || q.w > kVmapMaxW)
        return hipErrorInvalidValue;
    VmapParams p = q;
    const dim3 rows4((p.h + 3) / 4), block(256);
    if (p.w <= vmap_wave_max_w(1)) {
        hipLaunchKernelGGL(dcte_vmap_row<1>, rows4, block, 0, s, p);
    } else if (p.w <= vmap_wave_max_w(4)) {
        hipLaunchKernelGGL(dcte_vmap_row<4>, rows4, block, 0, s, p);
    } else {
        p.blk = (p.w + kWideBlocks - 1) / kWideBlocks;
        hipLaunchKernelGGL(dcte_vmap_wide, dim3(p.h), dim3(64), 0, s, p);
    }
    return hipGetLastError();
}

hipError_t launch_vmap_render(const RenderParams& p, hipStream_t s)
{
    if (p.w < 1 || p.h < 1 || p.w + p.delta < 1 || p.w > kVmapMaxW) return hipErrorInvalidValue;
    const dim3 grid((p.h + 3) / 4), block(256);
    const bool dword = p.bpp == 4 &&
                       ((reinterpret_cast<uintptr_t>(p.px) | reinterpret_cast<uintptr_t>(p.out) |
                         (uintptr_t)p.rowstride | (uintptr_t)p.out_rowstride) & 3u) == 0;
    switch (p.bpp) {
    case 1: hipLaunchKernelGGL((dcte_vmap_render<1, false>), grid, block, 0, s, p); break;
    case 3: hipLaunchKernelGGL((dcte_vmap_render<3, false>), grid, block, 0, s, p); break;
    case 4:
        if (dword) hipLaunchKernelGGL((dcte_vmap_render<4, true>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((dcte_vmap_render<4, false>), grid, block, 0, s, p);
        break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_vmap_seams_u8(const RenderParams& p, hipStream_t s)
{
    if (p.w < 1 || p.h < 1 || p.depth < 0 || p.w > kVmapMaxW) return hipErrorInvalidValue;
    const dim3 grid(p.h), block(256);
    switch (p.bpp) {
    case 1: hipLaunchKernelGGL(dcte_vmap_seams_u8<1>, grid, block, 0, s, p); break;
    case 3: hipLaunchKernelGGL(dcte_vmap_seams_u8<3>, grid, block, 0, s, p); break;
    case 4: hipLaunchKernelGGL(dcte_vmap_seams_u8<4>, grid, block, 0, s, p); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace dcte
