// mrts_aux.hip — gfx950 kernels beside the step: the one-hot and record renderers, the mask widening, the forward
// model's game copies, the evaluation function and the packed observation rows.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define MRTS_UNIT 2
#include "mrts_device.h"

namespace mrts {
// MicroRTS-Py GridnetVecEnv observation encoding (gym_microrts `_encode_obs`: clip each plane to
// [0, n_k - 1], one-hot, channels-last): int32 obs [S][C][H][W] -> uint8 [S][H][W][F] with plane sizes
// n = {5 hp, 5 resources, 3 owner, ntypes + 1 type, 6 action, 2 terrain, 2 per PO visibility plane}.
// One thread per cell over the flattened (slot, cell) index; a block's 256 cells x F bytes are
// composed in LDS and leave as aligned 16-byte stores (256 * F is a multiple of 16 for any F).
struct OneHotParams {
    const int32_t* obs;
    uint8_t* out;
    int32_t n_cells, HW, C, F;
    int32_t sizes[8], offs[8];
};
__global__ __launch_bounds__(256) void k_onehot(OneHotParams Q) {
    __shared__ __align__(16) uint8_t buf[256 * 40];
    const int t = (int)threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * 256, i = i0 + t;
    const int F = Q.F;
    for (int k = t; k < 256 * F / 4; k += 256) ((uint32_t*)buf)[k] = 0u;
    __syncthreads();
    if (i < Q.n_cells) {
        const int64_t slot = i / Q.HW;
        const int c = (int)(i - slot * Q.HW);
        const int32_t* o = Q.obs + slot * Q.C * Q.HW + c;
        for (int p = 0; p < Q.C; p++) {
            const int v = min(max(o[(int64_t)p * Q.HW], 0), Q.sizes[p] - 1);
            buf[t * F + Q.offs[p] + v] = 1;
        }
    }
    __syncthreads();
    const int64_t ncell = min((int64_t)256, (int64_t)Q.n_cells - i0);
    const int64_t nbytes = ncell * F, n16 = nbytes / 16;
    uint8_t* dst = Q.out + i0 * F;
    for (int64_t k = t; k < n16; k += 256) ((uint4*)dst)[k] = ((const uint4*)buf)[k];
    for (int64_t k = 16 * n16 + t; k < nbytes; k += 256) dst[k] = buf[k];
}
// the one definition of the encoding's table: plane p's one-hot size and its first byte in a cell's F bytes (F returned)
static int oneHotTable(int C, int ntypes, int32_t sizes[8], int32_t offs[8]) {
    const int base[6] = {5, 5, 3, ntypes + 1, 6, 2};
    int f = 0;
    for (int p = 0; p < 8; p++) {
        sizes[p] = p < 6 ? base[p] : 2;
        offs[p] = f;
        if (p < C) f += sizes[p];
    }
    return f;
}
hipError_t launchOneHot(const int32_t* obs, uint8_t* out, int n_slots, int HW, int C, int ntypes, hipStream_t stream) {
    OneHotParams Q;
    Q.obs = obs;
    Q.out = out;
    Q.n_cells = n_slots * HW;
    Q.HW = HW;
    Q.C = C;
    const int f = Q.F = oneHotTable(C, ntypes, Q.sizes, Q.offs);
    if (C > 8 || f > 40 || ((uintptr_t)out & 15)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_onehot, dim3((unsigned)((Q.n_cells + 255) / 256)), dim3(256), 0, stream, Q);
    return hipGetLastError();
}

// int32 copy of a uint8 mask buffer (the Java int[][][][] layout), 16 mask bytes per thread
__global__ __launch_bounds__(256) void k_widen(const uint8_t* __restrict__ in, int32_t* __restrict__ out, size_t n) {
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 16;
    if (i + 16 <= n) {
        const uint4 v = *(const uint4*)(in + i);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 4; q++)
            *(int4*)(out + i + 4 * q) = make_int4((int)(w[q] & 0xFF), (int)((w[q] >> 8) & 0xFF), (int)((w[q] >> 16) & 0xFF),
                                                  (int)(w[q] >> 24));
    } else {
        for (size_t k = i; k < n; k++) out[k] = in[k];
    }
}
hipError_t launchWiden(const uint8_t* in, int32_t* out, size_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (((uintptr_t)in & 15) || ((uintptr_t)out & 15)) return hipErrorInvalidValue;
    const size_t threads = (n + 15) / 16;
    hipLaunchKernelGGL(k_widen, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, in, out, n);
    return hipGetLastError();
}
// ---------------------------------------------------------------- forward model
// GameState.clone() (rts/GameState.java:591-610) of pairs (dst game, src game): units, players,
// time, the cancel counter and the assignments (LinkedHashMap order = the sequence numbers) travel;
// the dst game keeps its own random streams (Sampler.generator / GameState.r / UnitAction.r are
// JVM-global, not part of a GameState), its kind (playout policies), and its mask row sets (they
// describe the dst handle's mask buffer).  One block of 256 threads per pair.
// Receiver side of the compact observation exchange: the records of n_ranks x n_games games (rank r's
// game g at rec + r * rank_stride + g * recWords(units) words) back into both player slots'
// observation planes — GameState.getVectorObservation (rts/GameState.java:922-968), the owner plane
// per viewing player (:947-949), the terrain plane from the local handle's map of game g (every rank
// holds the same maps per game index).  out = [n_ranks][2 * n_games][C][HW] as uint8 (out_bytes 1)
// or int32 (4).  One wave per game: the units paint a byte image in LDS, then each lane stores 4 cells
// per plane.  HW <= 256, HW % 4 == 0 (the host checks).
// A record whose overflow bit is set (its game had more units than the record holds) renders without
// the missing units: the kernel then sets *err (mrts_render_status reports it).
__global__ __launch_bounds__(64) void k_render_records(const KStatic* __restrict__ PS, const uint32_t* __restrict__ rec,
                                                       int units, int64_t rank_stride, void* __restrict__ out, int out_bytes,
                                                       int32_t* __restrict__ err) {
    __shared__ uint32_t imgw[5 * 256 / 4];
    uint8_t* img = (uint8_t*)imgw;
    const KStatic& P = *PS;
    const int g = (int)blockIdx.x, r = (int)blockIdx.y, l = (int)threadIdx.x, HW = P.HW, C = P.C, G = P.n_games;
    const uint32_t* rc = rec + (size_t)r * (size_t)rank_stride + (size_t)g * recWords(units, false);
    for (int i = l; i < 5 * HW / 4; i += 64) imgw[i] = 0u;
    const uint32_t hdr = rc[0];
    if (l == 0 && (hdr >> 31)) *err = 1;  // a vector store from one lane (rare)
    __syncthreads();
    const int n = min((int)(hdr & 0xFFFFu), units);
    for (int i = l; i < n; i += 64) {
        const uint32_t w = rc[1 + i];
        const int c = (int)(w & 0xFFu);
        if (c >= HW) continue;  // (a foreign buffer: no LDS write out of range)
        img[c] = (uint8_t)(w >> 8);
        img[HW + c] = (uint8_t)(w >> 16);
        img[2 * HW + c] = (uint8_t)((w >> 27) & 3u);
        img[3 * HW + c] = (uint8_t)((w >> 24) & 7u);
        img[4 * HW + c] = (uint8_t)(w >> 29);
    }
    __syncthreads();
    const uint32_t* terr = (const uint32_t*)(P.tmpl + P.tmpl_off[g] + T_TERR);
    const size_t slot0 = (size_t)r * 2 * G + 2 * (size_t)g;
    for (int c4 = 4 * l; c4 < HW; c4 += 256) {
        uint32_t pw[6];
#pragma unroll
        for (int q = 0; q < 5; q++) pw[q] = imgw[(q * HW + c4) >> 2];
        const uint32_t t = terr[c4 >> 2];  // walls: non-zero terrain bytes
        uint32_t tw = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) tw |= (((t >> (8 * j)) & 0xFFu) ? 1u : 0u) << (8 * j);
        pw[5] = tw;
#pragma unroll
        for (int i = 0; i < 2; i++) {
#pragma unroll
            for (int q = 0; q < 6; q++) {
                uint32_t w = pw[q];
                if (i == 1 && q == 2) {  // the other player's owners: 1 <-> 2, 0 stays
                    uint32_t x = 0;
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const uint32_t b = (w >> (8 * j)) & 0xFFu;
                        x |= (b ? 3u - b : 0u) << (8 * j);
                    }
                    w = x;
                }
                const size_t off = ((slot0 + i) * C + q) * (size_t)HW + c4;
                if (out_bytes == 1) {
                    *(uint32_t*)((uint8_t*)out + off) = w;
                } else {
                    st4<true>((int32_t*)out + off, (int)(w & 0xFFu), (int)((w >> 8) & 0xFFu), (int)((w >> 16) & 0xFFu),
                              (int)(w >> 24));
                }
            }
        }
    }
}
// The same for partially observable handles (PartiallyObservableGameState.getVectorObservation,
// rts/PartiallyObservableGameState.java:82-154, as Game::writeObsPO renders it): per view p, the last
// unit of p's snapshot on each cell (list order) gives planes 0-4 — its live hp, resources, owner
// relative to p, type, and the action type p's snapshot saw — plane 5 the map's walls, planes 6 / 7
// whether a sight disk of one of the view's units owned by p / by the other player covers the cell.
// out = [n_ranks][2 * n_games][8][HW] as int8 (out_bytes 1: a dead unit's hp can be negative) or int32.
// One block of 256 threads per game and rank; LDS: the per-view cell owners (2 x HW words), sight rows
// (2 views x 2 x H x (W + 31) / 32 words) and the record itself (the per-cell lookups stay on chip).
// HW % 4 == 0 (the host checks).
__global__ __launch_bounds__(256) void k_render_records_po(const KStatic* __restrict__ PS, const uint32_t* __restrict__ rec,
                                                           int units, int64_t rank_stride, void* __restrict__ out, int out_bytes,
                                                           int32_t* __restrict__ err) {
    extern __shared__ __align__(16) uint32_t lds[];
    const KStatic& P = *PS;
    const int g = (int)blockIdx.x, r = (int)blockIdx.y, t = (int)threadIdx.x;
    const int H = P.H, W = P.W, HW = P.HW, C = P.C, G = P.n_games, NR = H * ((W + 31) >> 5);
    uint32_t* const sc = lds;             // [view][cell]: index + 1 of the view's last unit on the cell, 0 = none
    uint32_t* const rows = lds + 2 * HW;  // [view][own, other][NR]
    uint32_t* const rc = rows + 4 * NR;   // the record (1 + 2 x units words)
    const uint32_t* rg = rec + (size_t)r * (size_t)rank_stride + (size_t)g * recWords(units, true);
    const int n = min((int)(rg[0] & 0xFFFFu), units);
    if (t == 0 && (rg[0] >> 31)) *err = 1;  // overflow: units or an hp / resource value missing
    for (int i = t; i < 2 * HW + 4 * NR; i += 256) lds[i] = 0u;
    for (int i = t; i < 1 + 2 * n; i += 256) rc[i] = rg[i];
    __syncthreads();
    const int SM = P.utt.maxSight;
    const bool rowPaint = W <= 32 && SM <= 15;  // one word per sight row, table half-widths
    for (int i = t; i < n; i += 256) {  // the views' last unit per cell; and the sight disks (general maps)
        const uint32_t w0 = rc[1 + 2 * i], w1 = rc[2 + 2 * i];
        const int c = (int)(w0 & 0xFFFFu), ty = (int)(w1 & 15u) - 1, pl = (int)((w1 >> 4) & 3u) - 1;
        const uint32_t sb = (c < HW && ty >= 0 && ty < MAX_TYPES) ? (w1 >> 8) & 0xFFu : 0u;  // (a foreign buffer: no LDS write out of range)
        const int x = c % W, y = c / W;
        for (int p = 0; p < 2; p++) {
            if (!((sb >> p) & 1u)) continue;
            atomicMax(&sc[p * HW + c], (uint32_t)(i + 1));
            if (pl >= 0 && !rowPaint)
                paintDiskRows(rows + (2 * p + (pl == p ? 0 : 1)) * NR, H, W, x, y, P.utt.sight[ty], P.utt.diskLo[ty],
                              P.utt.diskHi[ty]);
        }
    }
    if (rowPaint) {
        // every (unit, row offset) pair on its own thread: 8 units x 32 row offsets per pass (2 SM + 1 <= 31),
        // one atomicOr per view the unit is in — not one thread looping over a unit's rows
        const int dy = (t & 31) - SM;
        for (int i = t >> 5; i < n; i += 8) {
            const uint32_t w0 = rc[1 + 2 * i], w1 = rc[2 + 2 * i];
            const int c = (int)(w0 & 0xFFFFu), ty = (int)(w1 & 15u) - 1, pl = (int)((w1 >> 4) & 3u) - 1;
            const uint32_t sb = (c < HW && ty >= 0 && ty < MAX_TYPES && pl >= 0) ? (w1 >> 8) & 3u : 0u;
            const int ady = dy < 0 ? -dy : dy, sr = sb ? P.utt.sight[ty] : -1;
            const int x = c % W, yy = c / W + dy;
            if (ady <= sr && yy >= 0 && yy < H) {
                const uint32_t half = ((ady < 8 ? P.utt.diskLo[ty] : P.utt.diskHi[ty]) >> (4 * (ady & 7))) & 0xFu;
                const int x0 = max(0, x - (int)half), x1 = min(W - 1, x + (int)half);
                const uint32_t b = ((2u << (x1 - x0)) - 1u) << x0;  // columns x0..x1 (x1 - x0 = 31: 2u << 31 wraps to 0)
                if (sb & 1u) atomicOr(&rows[(pl == 0 ? 0 : 1) * NR + yy], b);
                if (sb & 2u) atomicOr(&rows[(2 + (pl == 1 ? 0 : 1)) * NR + yy], b);
            }
        }
    }
    __syncthreads();
    const uint32_t* terr = (const uint32_t*)(P.tmpl + P.tmpl_off[g] + T_TERR);
    const int WPR = (W + 31) >> 5;
    for (int c4 = 4 * t; c4 < HW; c4 += 4 * 256) {
        const uint32_t tw = terr[c4 >> 2];  // walls: non-zero terrain bytes
        for (int p = 0; p < 2; p++) {
            int v[8][4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int c = c4 + j, x = c % W, y = c / W;
                const uint32_t s = sc[p * HW + c];
                const uint32_t w0 = s ? rc[2 * s - 1] : 0u, w1 = s ? rc[2 * s] : 0u;
                const int pl = (int)((w1 >> 4) & 3u) - 1, ca = (int)((w1 >> (10 + 3 * p)) & 7u);
                v[0][j] = s ? (int)(int8_t)(uint8_t)(w0 >> 16) : 0;
                v[1][j] = s ? (int)(w0 >> 24) : 0;
                v[2][j] = (s && pl >= 0) ? ((pl + p) % 2) + 1 : 0;
                v[3][j] = s ? (int)(w1 & 15u) : 0;
                v[4][j] = (s && ca) ? ca - 1 : 0;
                v[5][j] = ((tw >> (8 * j)) & 0xFFu) ? 1 : 0;
                v[6][j] = (int)((rows[(2 * p) * NR + y * WPR + (x >> 5)] >> (x & 31)) & 1u);
                v[7][j] = (int)((rows[(2 * p + 1) * NR + y * WPR + (x >> 5)] >> (x & 31)) & 1u);
            }
            const size_t slot = (size_t)r * 2 * G + 2 * (size_t)g + p;
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const size_t off = (slot * C + q) * (size_t)HW + c4;
                if (out_bytes == 1)
                    *(uint32_t*)((uint8_t*)out + off) = (uint32_t)(v[q][0] & 0xFF) | ((uint32_t)(v[q][1] & 0xFF) << 8) |
                                                         ((uint32_t)(v[q][2] & 0xFF) << 16) | ((uint32_t)(v[q][3] & 0xFF) << 24);
                else
                    st4<true>((int32_t*)out + off, v[q][0], v[q][1], v[q][2], v[q][3]);
            }
        }
    }
}
// A learner's batch straight from the exchanged records, in the layout it consumes: the
// MicroRTS-Py encoding of the observation (gym_microrts `_encode_obs`, as k_onehot: clip each plane, one-hot,
// channels last) of n_sel samples: sample i is slot sel[i] (global index r * n_slots + slot over every rank's
// slots) of the step whose rank-0 records start at rec + step_off[2i] with rank stride step_off[2i + 1] (the
// rollout's step_offsets row; null: rec and rank_stride) — a minibatch of (step, slot) pairs from a whole
// rollout window in one launch, with no int32 / uint8 planes of all ranks in between.  Full observability.  One 256-thread block per selected
// slot: its game's record paints the 5 dynamic planes as bytes in LDS (as k_render_records), each cell's
// F one-hot bytes are composed in LDS, and the slot's H x W x F bytes leave as aligned 16-byte stores.
// out = [n_sel][H][W][F] uint8 (HW * F % 16 == 0, the host checks).
__global__ __launch_bounds__(256) void k_render_records_onehot(const KStatic* __restrict__ PS, const uint32_t* __restrict__ rec,
                                                               int units, int64_t rank_stride, const int32_t* __restrict__ sel,
                                                               const int64_t* __restrict__ step_off, uint8_t* __restrict__ out,
                                                               OneHotParams Q, int32_t* __restrict__ err, int64_t rec_words,
                                                               int n_ranks) {
    __shared__ uint32_t imgw[5 * 256 / 4];
    __shared__ __align__(16) uint8_t buf[256 * 40];
    uint8_t* img = (uint8_t*)imgw;
    const KStatic& P = *PS;
    const int t = (int)threadIdx.x, HW = P.HW, S = 2 * P.n_games, F = Q.F;
    const int gs = sel[blockIdx.x];
    const int r = gs / S, slot = gs - r * S, g = slot >> 1, p = slot & 1;
    const int64_t o = step_off ? step_off[2 * blockIdx.x] : 0, rs = step_off ? step_off[2 * blockIdx.x + 1] : rank_stride;
    // a sample outside the buffer (a bad sel index or step_off row): a zero image and the render flag
    // (mrts_render_status), never a read past the receive buffer.  Block-uniform: the whole block returns.
    const int64_t at = o + (int64_t)r * rs + (int64_t)g * recWords(units, false);
    if (gs < 0 || r >= n_ranks || o < 0 || rs < 0 || at + recWords(units, false) > rec_words) {
        if (t == 0) *err = 1;
        uint4* dz = (uint4*)(out + (size_t)blockIdx.x * HW * F);
        for (int k = t; k < HW * F / 16; k += 256) dz[k] = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    const uint32_t* rc = rec + at;
    for (int i = t; i < 5 * HW / 4; i += 256) imgw[i] = 0u;
    for (int k = t; k < HW * F / 4; k += 256) ((uint32_t*)buf)[k] = 0u;
    const uint32_t hdr = rc[0];
    if (t == 0 && (hdr >> 31)) *err = 1;  // overflow (mrts_render_status)
    __syncthreads();
    const int n = min((int)(hdr & 0xFFFFu), units);
    for (int i = t; i < n; i += 256) {
        const uint32_t w = rc[1 + i];
        const int c = (int)(w & 0xFFu);
        if (c >= HW) continue;
        img[c] = (uint8_t)(w >> 8);
        img[HW + c] = (uint8_t)(w >> 16);
        img[2 * HW + c] = (uint8_t)((w >> 27) & 3u);  // player + 1 (0 = none)
        img[3 * HW + c] = (uint8_t)((w >> 24) & 7u);
        img[4 * HW + c] = (uint8_t)(w >> 29);
    }
    __syncthreads();
    const uint8_t* terr = (const uint8_t*)(P.tmpl + P.tmpl_off[g] + T_TERR);
    for (int c = t; c < HW; c += 256) {
        const int pl1 = img[2 * HW + c];  // owner plane of slot p: ((player + p) % 2) + 1
        const int v[6] = {img[c], img[HW + c], pl1 ? ((pl1 - 1 + p) & 1) + 1 : 0, img[3 * HW + c], img[4 * HW + c],
                          terr[c] ? 1 : 0};
#pragma unroll
        for (int q = 0; q < 6; q++) buf[c * F + Q.offs[q] + min(max(v[q], 0), Q.sizes[q] - 1)] = 1;
    }
    __syncthreads();
    uint4* dst = (uint4*)(out + (size_t)blockIdx.x * HW * F);
    for (int k = t; k < HW * F / 16; k += 256) dst[k] = ((const uint4*)buf)[k];
}
hipError_t launchRenderRecordsOneHot(const KStatic& hs, const KStatic* ds, const uint32_t* rec, int64_t rec_words, int n_ranks,
                                     int units, int64_t rank_stride, const int32_t* sel, const int64_t* step_off, int n_sel,
                                     uint8_t* out, int32_t* err, hipStream_t stream) {
    OneHotParams Q{};
    const int f = Q.F = oneHotTable(6, hs.utt.ntypes, Q.sizes, Q.offs);
    if (hs.partial_obs || hs.HW > 256 || f > 40 || ((size_t)hs.HW * f) % 16 || ((uintptr_t)out & 15)) return hipErrorInvalidValue;
    if (n_sel <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_render_records_onehot, dim3((unsigned)n_sel), dim3(256), 0, stream, ds, rec, units, rank_stride, sel,
                       step_off, out, Q, err, rec_words, n_ranks);
    return hipGetLastError();
}
hipError_t launchRenderRecords(const KStatic& hs, const KStatic* ds, const uint32_t* rec, int units, int n_ranks,
                               int64_t rank_stride, void* out, int out_bytes, int32_t* err, hipStream_t stream) {
    if (hs.partial_obs) {
        const size_t lds = 4 * (size_t)(2 * hs.HW + 4 * hs.H * ((hs.W + 31) / 32) + recWords(units, true));
        hipLaunchKernelGGL(k_render_records_po, dim3((unsigned)hs.n_games, (unsigned)n_ranks), dim3(256), lds, stream, ds, rec,
                           units, rank_stride, out, out_bytes, err);
    } else {
        hipLaunchKernelGGL(k_render_records, dim3((unsigned)hs.n_games, (unsigned)n_ranks), dim3(64), 0, stream, ds, rec, units,
                           rank_stride, out, out_bytes, err);
    }
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void k_copy_games(int32_t* __restrict__ dst, const int32_t* __restrict__ src,
                                                    const int32_t* __restrict__ pairs, int n_dst, int n_src,
                                                    int words, int src_words, int maskLo, int maskHi) {
    const int d = pairs[2 * blockIdx.x], s = pairs[2 * blockIdx.x + 1];
    if (d < 0 || d >= n_dst || s < 0 || s >= n_src) return;
    int32_t* o = dst + (size_t)d * words;
    const int32_t* i = src + (size_t)s * src_words;  // a source with LightRush games: longer blocks, same leading words
    for (int w = threadIdx.x; w < words; w += 256) {
        const bool keep = (w >= H_RNG_CANCEL && w <= H_KIND) || (w >= maskLo && w < maskHi);
        if (!keep) o[w] = w == H_STEPS ? 0 : i[w];
    }
}
hipError_t launchCopyGames(int32_t* dst, const int32_t* src, const int32_t* pairs, int n, int n_dst, int n_src,
                           int CAP, int HW, int src_words, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    // The destination's stride is stateWords: mrts_copy_games' destination is a forward-model handle (checkCopy), and
    // mrts_create refuses LightRush there, so its blocks never carry bot memory.  A destination with longer blocks
    // would need its own stride here (and a decision on what a copied game's bot memory is).
    const int lo = H_WORDS + N_ARRAYS * CAP;
    hipLaunchKernelGGL(k_copy_games, dim3((unsigned)n), dim3(256), 0, stream, dst, src, pairs, n_dst, n_src,
                       stateWords(CAP, HW), src_words, lo, lo + 2 * maskWords(HW));
    return hipGetLastError();
}

// SimpleSqrtEvaluationFunction3.evaluate(maxplayer, 1 - maxplayer, gs)
// (ai/evaluation/SimpleSqrtEvaluationFunction3.java:24-44), Java float semantics: the unit loop runs
// in list order, `score += res * 10f` is a float add, `score += 40f * cost * Math.sqrt(hp / maxHp)`
// (integer division) is a double add rounded back to float; no contraction into FMAs.  One wave per
// game: lanes load 64 units at a time, every lane runs the same ordered sum over readlane values.
__global__ __launch_bounds__(64) void k_evaluate(const KStatic* __restrict__ PS, const int32_t* __restrict__ state,
                                                 int words, int CAP, int maxplayer, float* __restrict__ out) {
#pragma clang fp contract(off)
    const KStatic& P = *PS;
    const int32_t* s = state + (size_t)blockIdx.x * words;
    const int nu = uni(s[H_NU]);
    const int l = lane_id();
    float score[2];
    bool any[2] = {false, false};
    score[0] = __fmul_rn((float)uni(s[H_RES0]), 20.0f);
    score[1] = __fmul_rn((float)uni(s[H_RES1]), 20.0f);
    for (int o0 = 0; o0 < nu; o0 += 64) {
        const int o = o0 + l;
        uint32_t c = UC_DEAD;
        int hpv = 0, rv = 0;
        if (o < nu) {
            c = (uint32_t)s[H_WORDS + A_UC * CAP + o];
            hpv = s[H_WORDS + A_HP * CAP + o];
            rv = s[H_WORDS + A_RES * CAP + o];
        }
        const int n = min(64, nu - o0);
        for (int k = 0; k < n; k++) {
            const uint32_t ck = (uint32_t)rl((int)c, k);
            if (ck & UC_DEAD) continue;
            const int p = uplay(ck);
            if (p != 0 && p != 1) continue;
            const int typ = utyp(ck);
            const int h = rl(hpv, k), r = rl(rv, k);
            float sc = score[p];
            sc = __fadd_rn(sc, __fmul_rn((float)r, 10.0f));
            const double bonus = __dmul_rn((double)__fmul_rn(40.0f, (float)P.utt.cost[typ]),
                                           __builtin_sqrt((double)(h / P.utt.hp[typ])));
            sc = (float)__dadd_rn((double)sc, bonus);
            score[p] = sc;
            any[p] = true;
        }
    }
    const float s1 = any[maxplayer] ? score[maxplayer] : 0.0f;
    const float s2 = any[1 - maxplayer] ? score[1 - maxplayer] : 0.0f;
    const float tot = __fadd_rn(s1, s2);
    const float v = tot == 0.0f ? 0.5f : __fsub_rn(__fdiv_rn(__fmul_rn(2.0f, s1), tot), 1.0f);
    if (l == 0) out[blockIdx.x] = v;
}
hipError_t launchEvaluate(const KStatic& hs, const KStatic* ds, int maxplayer, float* out, hipStream_t stream) {
    // the handle's block stride: a handle with a LightRush game has the bot memory after every state block
    const int words = hs.bot_off ? hs.bot_off + botWords(hs.CAP) : stateWords(hs.CAP, hs.HW);
    hipLaunchKernelGGL(k_evaluate, dim3((unsigned)hs.n_games), dim3(64), 0, stream, ds, hs.state, words, hs.CAP, maxplayer, out);
    return hipGetLastError();
}

// ---------------------------------------------------------------- packed observation rows
// include/mrts.h "Packed observation rows": what a rollout keeps of an observation [C][HW] — its occupied cells (any
// of planes 0-4 non-zero) as two words each, and planes 5.. as bitmaps.
constexpr int OBS_STG = 192;    // cells k_obs_pack stages in LDS between flushes (a chunk adds at most 64)
constexpr int OBS_BMSEG = 128;  // bitmap words per plane it stages between flushes (64 chunks; even)
constexpr int OBS_TILE = 256;   // cells of a reader's tile (one thread each)
DEV int wordAlign(const void* p) { return (int)(((uintptr_t)p >> 2) & 3); }
DEV int obsClamp(int v, int lo, int hi, bool& clamped) {
    const int c = min(max(v, lo), hi);
    clamped |= c != v;
    return c;
}
// the staged words [w0, w0 + nw) of every bitmap to the row (brow: its first bitmap word)
template <int C>
DEV void obsFlushBitmaps(int32_t (*bm)[4 + OBS_BMSEG + 4], int32_t* brow, int MW, int w0, int nw, int lane) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < C - 5; q++) {
        int32_t* g = brow + (size_t)q * MW + w0;
        const int ab = wordAlign(g);
        headFlush(bm[q], g - ab, ab, nw, lane);
    }
    __syncthreads();
}
// One wave per row.  Per 64 cells every lane loads its cell's C plane values (unconditional loads, in flight
// together); one ballot of "any of planes 0-4 non-zero" marks the occupied lanes, whose place in the row is the count
// before the chunk plus the occupied lanes below; a ballot per plane 5.. is two bitmap words.  Cells and bitmaps are
// composed in LDS and leave as dwordx4 (headFlush), count word and zero tail included; a row of more cells than
// OBS_STG, or of more bitmap words than OBS_BMSEG, flushes in between.  Row starts are only 4-byte aligned.
template <int C>
__global__ __launch_bounds__(64) void k_obs_pack(ObsPackParams P) {
    __shared__ __align__(16) int32_t stg[4 + 1 + 2 * OBS_STG + 3];
    __shared__ __align__(16) int32_t bm[C - 5][4 + OBS_BMSEG + 4];
    const int lane = (int)threadIdx.x, row = (int)blockIdx.x, HW = P.HW, MW = (HW + 31) / 32;
    const int32_t* o = P.obs + (size_t)row * C * HW;
    int32_t* orow = (int32_t*)P.packed_out + (size_t)row * (size_t)P.words;
    int32_t* brow = orow + 1 + 2 * P.cap;
    // staged: the row's words [r0, r0 + rn) at stg[a + (word - r0)], orow + r0 - a 16-byte aligned; bitmap words
    // [w0, w0 + OBS_BMSEG) of plane 5 + q at bm[q][its own alignment + (word - w0)]
    int total = 0, r0 = 0, rn = 1, a = wordAlign(orow), w0 = 0;
    bool lossy = false;
    for (int c0 = 0; c0 < HW; c0 += 64) {
        const int c = c0 + lane;
        const bool in = c < HW;
        int v[C];
#pragma unroll
        for (int p = 0; p < C; p++) v[p] = o[(size_t)p * HW + (in ? c : 0)];
        const bool occ = in && (v[0] | v[1] | v[2] | v[3] | v[4]) != 0;
        const uint64_t m = ballot(occ);
        const int bw = c0 >> 5;  // the chunk's first bitmap word
        if (bw >= w0 + OBS_BMSEG) {
            obsFlushBitmaps<C>(bm, brow, MW, w0, OBS_BMSEG, lane);
            w0 += OBS_BMSEG;
        }
#pragma unroll
        for (int p = 5; p < C; p++) {
            const uint64_t b = ballot(in && v[p] != 0);
            lossy |= in && (uint32_t)v[p] > 1u;
            if (lane == 0) {
                int32_t* s = bm[p - 5] + wordAlign(brow + (size_t)(p - 5) * MW + w0) + (bw - w0);
                s[0] = (int32_t)(uint32_t)b;
                if (bw + 1 < MW) s[1] = (int32_t)(uint32_t)(b >> 32);
            }
        }
        if (m == 0) continue;
        const int nc = __builtin_popcountll(m), keep = max(0, min(nc, P.cap - total));
        total += nc;
        if (keep == 0) continue;
        if (rn + 2 * keep > 1 + 2 * OBS_STG) {  // word 0 waits for the count
            __syncthreads();
            if (r0 == 0) headFlush(stg, orow - a, a + 1, rn - 1, lane);
            else headFlush(stg, orow + r0 - a, a, rn, lane);
            __syncthreads();
            r0 += rn;
            rn = 0;
            a = wordAlign(orow + r0);
        }
        const int pos = lanes_below(m);
        if (occ && pos < keep) {
            int32_t* s = stg + a + rn + 2 * pos;
            bool cl = false;
            const uint32_t hp = (uint32_t)obsClamp(v[0], -32768, 32767, cl) & 0xFFFFu;
            const uint32_t res = (uint32_t)obsClamp(v[1], 0, 65535, cl), ow = (uint32_t)obsClamp(v[2], 0, 3, cl);
            const uint32_t ty = (uint32_t)obsClamp(v[3], 0, 31, cl), ac = (uint32_t)obsClamp(v[4], 0, 7, cl);
            s[0] = (int32_t)((uint32_t)c | (ow << 16) | (ac << 18) | (ty << 21));
            s[1] = (int32_t)(hp | (res << 16));
            lossy |= cl;
        }
        rn += 2 * keep;
    }
    const bool flag = ballot(lossy) != 0 || total > P.cap;
    if (lane == 0) {
        const int32_t w = (int32_t)((uint32_t)total | (flag ? 0x80000000u : 0u));
        if (r0 == 0) stg[a] = w;
        else orow[0] = w;
        if (flag) atomicAdd(P.counters, 1ull);
    }
    __syncthreads();
    headFlush(stg, orow + r0 - a, a, rn, lane);
    const int t0 = r0 + rn, a2 = wordAlign(orow + t0);
    headFlush(nullptr, orow + t0 - a2, a2, 1 + 2 * P.cap - t0, lane);
    obsFlushBitmaps<C>(bm, brow, MW, w0, MW - w0, lane);
}

// The readers, one 256-thread block per (row, tile of OBS_TILE cells).  Output row r reads packed row index[r] (r
// without an index); an index outside the packed rows gives a zero output row and one bad read.  A stored count
// above cap reads cap cells; a stored cell outside the map is skipped and is one bad read (counted by the row's
// first tile).  Every tile looks at every kept cell and takes those inside it, so nothing depends on their order.
struct ObsRow {
    const uint32_t* w;  // the packed row, null: an index outside the packed rows
    uint32_t n;         // its kept cells
};
DEV ObsRow obsPackedRow(const ObsPackParams& P, int row, bool first) {
    const int64_t pr = P.index ? (int64_t)P.index[row] : (int64_t)row;
    ObsRow R = {nullptr, 0u};
    if (pr >= 0 && pr < (int64_t)P.n_packed) {
        R.w = P.packed + (size_t)pr * (size_t)P.words;
        R.n = min(R.w[0] & 0x7FFFFFFFu, (uint32_t)P.cap);
    } else if (first && threadIdx.x == 0) {
        atomicAdd(P.counters + 1, 1ull);
    }
    return R;
}
// The tile's kept cells into its per-cell words (cwA: word A >> 16, cwB: word B; zero = an empty cell), and the
// thread's own cell's bits of planes 5.. (bit q: plane 5 + q).  The first round's cell words and the bitmap words
// are loaded before the count is looked at — they lie inside the row whatever the count says (entry t < cap) — so
// a row costs one memory round after its index.
DEV uint32_t obsScatter(const ObsPackParams& P, ObsRow R, int t0, int ncell, uint32_t* cwA, uint32_t* cwB, bool first) {
    const int t = (int)threadIdx.x, MW = (P.HW + 31) / 32, c = t0 + min(t, ncell - 1);
    uint32_t i = (uint32_t)t, A = 0u, B = 0u, bw[3] = {0u, 0u, 0u};
    if (i < (uint32_t)P.cap) A = R.w[1 + 2 * (size_t)i], B = R.w[2 + 2 * (size_t)i];
#pragma unroll
    for (int q = 0; q < 3; q++)
        if (q < P.C - 5) bw[q] = R.w[1 + 2 * (size_t)P.cap + (size_t)q * MW + (c >> 5)];
    cwA[t] = 0u;
    cwB[t] = 0u;
    __syncthreads();
    while (i < R.n) {
        const uint32_t cell = A & 0xFFFFu, k = cell - (uint32_t)t0;  // (a cell below the tile wraps past ncell)
        if (cell >= (uint32_t)P.HW) {
            if (first) atomicAdd(P.counters + 1, 1ull);
        } else if (k < (uint32_t)ncell) {
            cwA[k] = A >> 16;
            cwB[k] = B;
        }
        i += OBS_TILE;
        if (i < R.n) A = R.w[1 + 2 * (size_t)i], B = R.w[2 + 2 * (size_t)i];
    }
    __syncthreads();
    return ((bw[0] >> (c & 31)) & 1u) | (((bw[1] >> (c & 31)) & 1u) << 1) | (((bw[2] >> (c & 31)) & 1u) << 2);
}
// int32 planes [n_rows][C][HW]: each plane's OBS_TILE words composed in LDS, then aligned 16-byte stores (headFlush)
__global__ __launch_bounds__(OBS_TILE) void k_obs_unpack(ObsPackParams P) {
    __shared__ uint32_t cwA[OBS_TILE], cwB[OBS_TILE];
    __shared__ __align__(16) int32_t sp[8][4 + OBS_TILE + 4];
    const int t = (int)threadIdx.x, row = (int)blockIdx.x, t0 = (int)blockIdx.y * OBS_TILE, HW = P.HW, C = P.C;
    const int ncell = min(OBS_TILE, HW - t0);
    const ObsRow R = obsPackedRow(P, row, blockIdx.y == 0);
    int32_t* orow = P.obs_out + (size_t)row * C * HW + t0;
    if (R.w) {
        const uint32_t bits = obsScatter(P, R, t0, ncell, cwA, cwB, blockIdx.y == 0);
        if (t < ncell) {
            const uint32_t x = cwA[t], B = cwB[t];
            const int v[5] = {(int)(int16_t)(uint16_t)(B & 0xFFFFu), (int)(B >> 16), (int)(x & 3u), (int)((x >> 5) & 31u),
                              (int)((x >> 2) & 7u)};
#pragma unroll
            for (int p = 0; p < 5; p++) sp[p][wordAlign(orow + (size_t)p * HW) + t] = v[p];
            for (int p = 5; p < C; p++) sp[p][wordAlign(orow + (size_t)p * HW) + t] = (int)((bits >> (p - 5)) & 1u);
        }
        __syncthreads();
    }
    for (int p = 0; p < C; p++) {
        int32_t* g = orow + (size_t)p * HW;
        const int ab = wordAlign(g);
        headFlush(R.w ? sp[p] : nullptr, g - ab, ab, ncell, t, OBS_TILE);
    }
}
// the one-hot encoding [n_rows][HW][F] (k_onehot's bytes on the tensor the row was packed from): each cell's F
// bytes composed in zeroed LDS by the cell's thread, then aligned 16-byte stores (headFlushBytes)
__global__ __launch_bounds__(OBS_TILE) void k_obs_onehot_packed(ObsPackParams P) {
    __shared__ uint32_t cwA[OBS_TILE], cwB[OBS_TILE];
    __shared__ __align__(16) uint8_t buf[16 + OBS_TILE * 40 + 16];
    const int t = (int)threadIdx.x, row = (int)blockIdx.x, t0 = (int)blockIdx.y * OBS_TILE, HW = P.HW, C = P.C, F = P.F;
    const int ncell = min(OBS_TILE, HW - t0), nb = ncell * F;
    const ObsRow R = obsPackedRow(P, row, blockIdx.y == 0);
    uint8_t* g = P.onehot_out + ((size_t)row * HW + t0) * F;
    const int ab = (int)((uintptr_t)g & 15);
    if (R.w) {
        for (int k = t; k < ((ab + nb + 15) >> 4); k += OBS_TILE) ((int4*)buf)[k] = make_int4(0, 0, 0, 0);
        const uint32_t bits = obsScatter(P, R, t0, ncell, cwA, cwB, blockIdx.y == 0);  // (its barriers also order the zeroing)
        if (t < ncell) {
            const uint32_t x = cwA[t], B = cwB[t];
            const int v[5] = {(int)(int16_t)(uint16_t)(B & 0xFFFFu), (int)(B >> 16), (int)(x & 3u), (int)((x >> 5) & 31u),
                              (int)((x >> 2) & 7u)};
            uint8_t* cellb = buf + ab + t * F;
#pragma unroll
            for (int p = 0; p < 5; p++) cellb[P.offs[p] + min(max(v[p], 0), P.sizes[p] - 1)] = 1;
            for (int p = 5; p < C; p++) cellb[P.offs[p] + ((bits >> (p - 5)) & 1u)] = 1;
        }
        __syncthreads();
    }
    headFlushBytes(R.w ? buf : nullptr, g - ab, ab, nb, t, OBS_TILE);
}
hipError_t launchObsPacked(int mode, ObsPackParams P, int ntypes, hipStream_t stream) {
    P.F = oneHotTable(P.C, ntypes, P.sizes, P.offs);
    if ((P.C != 6 && P.C != 8) || P.F > 40 || P.HW > OBS_MAX_CELLS || P.cap < 1 || P.cap > P.HW ||
        P.words != obsPackedWords(P.C, P.HW, P.cap) || !P.counters)
        return hipErrorInvalidValue;
    if (P.n_rows <= 0) return hipSuccess;
    const dim3 tiles((unsigned)P.n_rows, (unsigned)((P.HW + OBS_TILE - 1) / OBS_TILE));
    if (mode == OBS_PACK) {
        if (P.C == 6) hipLaunchKernelGGL(k_obs_pack<6>, dim3((unsigned)P.n_rows), dim3(64), 0, stream, P);
        else hipLaunchKernelGGL(k_obs_pack<8>, dim3((unsigned)P.n_rows), dim3(64), 0, stream, P);
    } else if (mode == OBS_UNPACK) {
        hipLaunchKernelGGL(k_obs_unpack, tiles, dim3(OBS_TILE), 0, stream, P);
    } else {
        if ((uintptr_t)P.onehot_out & 15) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_obs_onehot_packed, tiles, dim3(OBS_TILE), 0, stream, P);
    }
    return hipGetLastError();
}
}  // namespace mrts
