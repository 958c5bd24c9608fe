// mrts_device.h — the device helpers that more than one .hip unit uses: output stores, the packed unit words'
// accessors, cross-lane reads and reductions, the random streams and the sampled rows.  Included by mrts_kernels.hip,
// mrts_policy.hip and mrts_aux.hip only; what the step kernel alone uses stays in mrts_kernels.hip.
// A unit defines MRTS_UNIT (0 kernels, 1 policy, 2 aux) before including it: the audit build's records name the
// unit their line is in (laneAuditHit).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mrts_internal.h"
#include "mrts_launch.h"

using namespace mrts;

#define DEV __device__ __forceinline__

namespace {

constexpr int INF = 0x7FFFFFFF;
DEV int lane_id() { return (int)threadIdx.x; }
// Output stores.  WT = streaming (`nt`) stores, so output lines do not sit dirty in the XCD's L2
// until the end-of-kernel write-back.  Builtins, not inline asm: the wait-count and store-data
// hazard passes must see the stores.
typedef int32_t i32x4v __attribute__((ext_vector_type(4)));
typedef int32_t i32x4u __attribute__((ext_vector_type(4), aligned(4)));
typedef int32_t i32x3u __attribute__((ext_vector_type(3), aligned(4)));
template <bool WT>
DEV void st4(void* p, int a, int b, int c, int d) {  // 16-byte aligned
    const i32x4v v = {a, b, c, d};
    if (WT) __builtin_nontemporal_store(v, (i32x4v*)p);
    else *(i32x4v*)p = v;
}
template <bool WT>
DEV void st4u(void* p, int a, int b, int c, int d) {  // 4-byte aligned
    const i32x4u v = {a, b, c, d};
    if (WT) __builtin_nontemporal_store(v, (i32x4u*)p);
    else *(i32x4u*)p = v;
}
template <bool WT>
DEV void st3u(void* p, int a, int b, int c) {  // 4-byte aligned
    const i32x3u v = {a, b, c};
    if (WT) __builtin_nontemporal_store(v, (i32x3u*)p);
    else *(i32x3u*)p = v;
}
template <bool WT>
DEV void st1(int32_t* p, int a) {
    if (WT) __builtin_nontemporal_store(a, p);
    else *p = a;
}
// The store policy, measured on c3 / c5 / --mask-mode full (profiles/r12_summary.md).  Streaming stores for:
constexpr bool WT_OBS = true,        // full-observability planes (c3 +4.5 %, full masks +3 %)
               WT_MASK = false,      // delta mask records + policy rows (c3 -1.3 %)
               WT_FULLMASK = false,  // full-rewrite mask chunks (-15 %)
               WT_STATE = false,     // the state block (neutral)
               WT_POOBS = false;     // partially observable planes (c5 -18 %)
// Round 2 (profiles/round2_store_policy.md): write-through (`sc1`) buffer stores leave no line in the XCD's L2,
// so the next step's state and action-row reads (the same game runs on the same XCD every launch:
// tools/xcd_placement.py) keep theirs; `rsrc` = a raw buffer over the stored region (gfx9 descriptor word 3).
constexpr bool SC1_OBS = true,     // full-observability planes (c3 +3.2 %)
               SC1_POOBS = true,   // partially observable planes (c5 +3.4 %)
               SC1_MASK = false;   // delta mask records (byte-granular partial lines: c3 -5 %)
// The plane stores are written for this policy: where a writer has the sc1 form it calls st4sc1 (or the b32
// builtin) directly, which takes precedence over WT_OBS / WT_POOBS.
static_assert(WT_OBS && SC1_OBS && SC1_POOBS, "plane stores: sc1 buffer stores");
DEV __amdgpu_buffer_rsrc_t bufRsrc(void* base, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(base, (short)0, (int)bytes, 0x00020000);
}
DEV void st4sc1(__amdgpu_buffer_rsrc_t r, uint32_t byteOff, int a, int b, int c, int d) {
    const i32x4v v = {a, b, c, d};
    __builtin_amdgcn_raw_buffer_store_b128(v, r, (int)byteOff, 0, 16);
}
DEV int ux(uint32_t c) { return (int)(c & 0xFF); }
DEV int uy(uint32_t c) { return (int)((c >> 8) & 0xFF); }
DEV int utyp(uint32_t c) { return (int)((c >> 16) & 0xF); }
DEV int uplay(uint32_t c) { return (int)((c >> 20) & 3) - 1; }
DEV uint32_t pack_uc(int x, int y, int t, int p) {
    return (uint32_t)x | ((uint32_t)y << 8) | ((uint32_t)t << 16) | ((uint32_t)(p + 1) << 20);
}
DEV int ua_type(uint32_t a) { return (int)(a & 0xF); }
DEV int ua_ut(uint32_t a) { return (int)((a >> 4) & 0xF); }
DEV int ua_tx(uint32_t a) { return (int)((a >> 8) & 0xFF); }
DEV int ua_ty(uint32_t a) { return (int)((a >> 16) & 0xFF); }
DEV uint32_t pack_ua(int t, int ut, int tx, int ty) {
    return (uint32_t)t | ((uint32_t)ut << 4) | ((uint32_t)tx << 8) | ((uint32_t)ty << 16);
}
// UnitAction.DIRECTION_OFFSET_X/Y (rts/UnitAction.java:94-100); invalid directions move nowhere
DEV int dxo(int d) { return d == 1 ? 1 : (d == 3 ? -1 : 0); }
DEV int dyo(int d) { return d == 0 ? -1 : (d == 2 ? 1 : 0); }
DEV int clampdir(int d) { return (d >= 0 && d <= 3) ? d : ACT_INVALID; }

// Diagnostic build only (-DMRTS_LANE_AUDIT, `make audit`; tests/test_zz_lane_audit.py): every cross-lane read
// checks at run time that the lanes it reads are active where it executes — a readlane's source lane, every lane
// for the DPP reductions and ballots (which the code treats as whole-wave) — and records the source line of a
// violation in g_laneAudit (one vector store per lane, its own slot).  A readlane of an inactive lane returns
// whatever its register last held (the round-4 soak's stale PO value).  Not in libmrts.so.
// Every unit has its own g_laneAudit (no device linking); a record names its unit: line | MRTS_UNIT << 20 | kind << 24.
#ifdef MRTS_LANE_AUDIT
__device__ int32_t g_laneAudit[256];
DEV void laneAuditHit(int line, int kind) { g_laneAudit[threadIdx.x & 255] = line | (MRTS_UNIT << 20) | (kind << 24); }
DEV bool laneOn(int k) { return (__builtin_amdgcn_read_exec() >> k) & 1ull; }
DEV bool waveOn() { return __builtin_amdgcn_read_exec() == ~0ull; }
DEV int rlAudit(int v, int k, int line) {
    if (!laneOn(k)) laneAuditHit(line, 1);
    return __builtin_amdgcn_readlane(v, k);
}
#define rl(v, k) rlAudit((v), (k), __LINE__)
#define LANE_AUDIT_WAVE(kind)                              \
    do {                                                   \
        if (!waveOn()) laneAuditHit(__LINE__, (kind));     \
    } while (0)
#else
DEV int rl(int v, int k) { return __builtin_amdgcn_readlane(v, k); }
#define LANE_AUDIT_WAVE(kind) ((void)0)
#endif
// four int32 values (each within int16) as four packed int16
DEV uint2 pk16(int4 w) {
    return make_uint2(((uint32_t)w.x & 0xFFFFu) | ((uint32_t)w.y << 16), ((uint32_t)w.z & 0xFFFFu) | ((uint32_t)w.w << 16));
}
DEV int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
DEV uint32_t uniu(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
#ifdef MRTS_LANE_AUDIT
#define ballot(p) ballotAudit((p), __LINE__)
DEV uint64_t ballotAudit(bool p, int line) {
    if (!waveOn()) laneAuditHit(line, 3);
    return __ballot(p);
}
#else
DEV uint64_t ballot(bool p) { return __ballot(p); }
#endif
DEV int lanes_below(uint64_t m) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
}
// A game is one wave and its LDS is private to that wave: LDS operations of one wave execute in
// order, so a wave-scope fence (a compiler barrier, no instruction) orders them across lanes.
DEV void wsync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Whole-wave reductions with DPP (GFX9 row_bcast forms): quad swaps, half-row and row mirrors
// reduce each 16-lane row; row_bcast:15/31 chain the rows; lane 63 holds the result.
template <bool MIN>
DEV int wave_reduce(int v) {
    LANE_AUDIT_WAVE(2);
    const int id = MIN ? INF : 0;
    auto op = [](int a, int b) { return MIN ? min(a, b) : a + b; };
    v = op(v, __builtin_amdgcn_update_dpp(id, v, 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
    v = op(v, __builtin_amdgcn_update_dpp(id, v, 0x4E, 0xF, 0xF, false));   // quad_perm [2,3,0,1]
    v = op(v, __builtin_amdgcn_update_dpp(id, v, 0x141, 0xF, 0xF, false));  // row_half_mirror
    v = op(v, __builtin_amdgcn_update_dpp(id, v, 0x140, 0xF, 0xF, false));  // row_mirror
    v = op(v, __builtin_amdgcn_update_dpp(id, v, 0x142, 0xA, 0xF, false));  // row_bcast:15
    v = op(v, __builtin_amdgcn_update_dpp(id, v, 0x143, 0xC, 0xF, false));  // row_bcast:31
    return rl(v, 63);
}
// Inclusive prefix sum over the wave's lanes with DPP: row_shr 1/2/4/8 scan each 16-lane row
// (lanes shifted in from outside the row read 0), row_bcast:15 / :31 carry the row totals.
DEV int wave_incl_sum(int v) {
    LANE_AUDIT_WAVE(2);
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, false);  // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, false);  // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, false);  // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, false);  // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);  // row_bcast:15 -> rows 1, 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);  // row_bcast:31 -> rows 2, 3
    return v;
}
DEV int wave_min(int v) { return wave_reduce<true>(v); }
DEV int wave_sum(int v) { return wave_reduce<false>(v); }

// java.util.Random (48-bit LCG, JDK 8) — GameState.r / UnitAction.r / Sampler.generator, per game
struct JRand {
    uint64_t s;
    DEV int next(int bits) {
        s = (s * 0x5DEECE66DULL + 0xBULL) & ((1ULL << 48) - 1);
        return (int)(uint32_t)(s >> (48 - bits));
    }
    DEV int nextInt(int bound) {
        if ((bound & -bound) == bound) return (int)(((int64_t)bound * (int64_t)next(31)) >> 31);
        int bits, val;
        do {
            bits = next(31);
            val = bits % bound;
        } while ((int)((uint32_t)bits - (uint32_t)val + (uint32_t)(bound - 1)) < 0);
        return val;
    }
    DEV double nextDouble() { return (double)(((int64_t)next(26) << 27) + next(27)) * (1.0 / 9007199254740992.0); }
};
DEV uint64_t rng_of(int lo, int hi) { return (uint64_t)(uint32_t)lo | ((uint64_t)(uint32_t)hi << 32); }

// Snapshot byte per unit for PartiallyObservableGameState views (rts/PartiallyObservableGameState.java:35-54):
// bit p = unit is in player p's snapshot list; bits 2-4 / 5-7 = (snapshot UAA action type + 1), 0 = none.
DEV int snap_in(uint32_t b, int p) { return (b >> p) & 1; }
DEV int snap_act(uint32_t b, int p) { return (int)((b >> (2 + 3 * p)) & 7); }

// The unit-type table is read with lane-varying indices all over the step; an LDS copy turns those
// global loads into LDS reads.
constexpr int UTT_WORDS = (int)(sizeof(DevUtt) / 4);
constexpr int UTT_LDS = (int)((sizeof(DevUtt) + 15) & ~(size_t)15);
static_assert(sizeof(DevUtt) % 4 == 0 && UTT_WORDS <= 192, "DevUtt copy: 3 words per lane");

// a ^ b ^ k in one VALU instruction (gfx950's three-input bit op, truth table 0x96; the compiler emits
// two v_xor_b32 for it).  k MUST be wave-uniform (a Philox key word, in an SGPR): the "s" constraint would
// silently readfirstlane a per-lane value.  Other targets (ARCH overridden) take the plain C form.
DEV uint32_t xor3s(uint32_t a, uint32_t b, uint32_t k) {
#if defined(__gfx950__)
    uint32_t d;
    asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96" : "=v"(d) : "v"(a), "v"(b), "s"(k));
    return d;
#else
    return a ^ b ^ k;
#endif
}
// Philox4x32-10, the ten rounds unrolled (rolled, the loop carried two v_mov per round and the xors
// were not fused: 8 VALU per round against 4)
DEV void philox(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = xor3s((uint32_t)(p1 >> 32), c[1], k0), n1 = (uint32_t)p1;
        const uint32_t n2 = xor3s((uint32_t)(p0 >> 32), c[3], k1), n3 = (uint32_t)p0;
        c[0] = n0;
        c[1] = n1;
        c[2] = n2;
        c[3] = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}
DEV int pickBit(uint32_t r, uint64_t bitsv, int n) {
    const uint64_t m = n >= 64 ? ~0ull : ((1ull << n) - 1);
    bitsv &= m;
    const int cnt = __popcll(bitsv);
    if (cnt == 0) return -1;
    int k = (int)(((uint64_t)r * (uint32_t)cnt) >> 32);
    while (k--) bitsv &= bitsv - 1;
    return __builtin_ctzll(bitsv);
}
// one cell's action from its mask bits (lo/hi: mask slots 1..K-1 -> bit i-1), Philox counter
// (slot id, step, cell, 0)
// Masked-uniform random policy of one cell (the bench / rollout agent): mask slots 1..K-1 as bits
// (lo: slots 1..64, hi: 65..), Philox4x32-10 with key = seed, counter = (slot id, step, cell, 0)
// pickBit of a field of at most 32 bits (already masked): the same pick in 32-bit operations
DEV int pickBit32(uint32_t r, uint32_t bitsv) {
    const int cnt = __popc(bitsv);
    if (cnt == 0) return -1;
    int k = (int)__umulhi(r, (uint32_t)cnt);
    while (k--) bitsv &= bitsv - 1;
    return __builtin_ctz(bitsv);
}
// packFwd of a row with every value 0 (each parameter field holds value + 1)
constexpr uint32_t FWD_ZERO = (1u << 3) | (1u << 6) | (1u << 9) | (1u << 12) | (1u << 15) | (1u << 19);
// packed (optional): packFwd(a) of the drawn row, built from the picks (no field repacking)
// picks (optional): the picks themselves — the type (0 = none), the chosen type's parameter pick, the produce type
// The parameter comes from ONE pick over the chosen type's field, not one pick per case of a switch over the type:
// the lanes of a wave hold several types, and a switch runs its cases one after the other.
DEV void sampleBitsRaw(uint64_t seed, uint32_t step, uint32_t slotId, int ntypes, int K, uint64_t lo, uint64_t hi, int c,
                       int32_t a[7], uint32_t* packed = nullptr, int picks[3] = nullptr) {
    uint32_t ctr[4] = {slotId, step, (uint32_t)c, 0u};
    philox(ctr, (uint32_t)seed, (uint32_t)(seed >> 32));
    // mask slots 1..K-1 as bits of lo:hi (slot k -> bit k - 1): the type field is bits 0..5, the produce
    // types bits 22.., the direction fields bits 6 + 4 (t - 1).., the attack window bits 22 + ntypes..
    const int t = pickBit32(ctr[0], (uint32_t)lo & 63u);
    int pv = 0, ut = 0;
    if (t > 0 && t < 5) {
        // a direction: 4 bits at 2 + 4 t (below 32) — one 32-bit pick
        pv = pickBit32(ctr[1], ((uint32_t)lo >> (2 + 4 * t)) & 15u);
    } else if (t > 0) {
        // the attack window: K - 23 - ntypes bits from 22 + ntypes (across lo / hi), a 64-bit pick
        const int b = t == 5 ? 22 + ntypes : 2 + 4 * t, n = t == 5 ? K - 23 - ntypes : 4;
        uint64_t v = b >= 64 ? hi >> (b - 64) : ((lo >> b) | (hi << (64 - b)));
        v &= n >= 64 ? ~0ull : ((1ull << n) - 1);
        pv = pickBit(ctr[1], v, 64);
    }
    if (t == 4) ut = pickBit32(ctr[2], (uint32_t)(lo >> 22) & ((1u << ntypes) - 1u));
    a[0] = t > 0 ? t : 0;
    a[1] = t == 1 ? pv : 0;
    a[2] = t == 2 ? pv : 0;
    a[3] = t == 3 ? pv : 0;
    a[4] = t == 4 ? pv : 0;
    a[5] = ut;
    a[6] = t == 5 ? pv : 0;
    if (packed)
        *packed = FWD_ZERO + (uint32_t)(t > 0 ? t : 0) + (t > 0 ? (uint32_t)pv << (t == 5 ? 19 : 3 * t) : 0u) +
                  ((uint32_t)ut << 15);
    if (picks) {
        picks[0] = t > 0 ? t : 0;
        picks[1] = pv;
        picks[2] = ut;
    }
}

// Unmasked uniform random row (BASELINE config c2) of cell c of slot id slotId:
// type in [0, 6), the four directions in [0, 4), produce type in [0, ntypes), attack window index
// in [0, natt) — rows that reach every illegal -> NONE path of issueSafe.  Philox4x32-10, key =
// seed, counter = (slot id, step, cell, UNIFORM_TAG); ranges by multiply-shift of the 32-bit words.
constexpr uint32_t UNIFORM_TAG = 0x554E4946u;  // "UNIF": a stream apart from the masked policy's (word 3 = 0)
DEV void uniformRow(uint64_t seed, uint32_t step, uint32_t slotId, int c, int ntypes, int natt, int32_t a[7]) {
    uint32_t ctr[4] = {slotId, step, (uint32_t)c, UNIFORM_TAG};
    philox(ctr, (uint32_t)seed, (uint32_t)(seed >> 32));
    auto below = [](uint32_t r, int n) { return (int)(((uint64_t)r * (uint32_t)n) >> 32); };
    a[0] = below(ctr[0], 6);
    a[1] = (int)(ctr[1] & 3u);
    a[2] = (int)((ctr[1] >> 2) & 3u);
    a[3] = (int)((ctr[1] >> 4) & 3u);
    a[4] = (int)((ctr[1] >> 6) & 3u);
    a[5] = below(ctr[2], ntypes);
    a[6] = below(ctr[3], natt);
}

// Forwarded action word (H_FWD / stateFwdOff): the 7 values of a fused-policy row, which the sampler
// draws as type 0..5 and parameters -1..(field size - 1): type 3 bits, the four directions 3 bits
// each, produce type 4 bits, attack index 7 bits, each parameter stored + 1.
DEV uint32_t packFwd(const int32_t a[7]) {
    return ((uint32_t)a[0] & 7u) | (((uint32_t)(a[1] + 1) & 7u) << 3) | (((uint32_t)(a[2] + 1) & 7u) << 6) |
           (((uint32_t)(a[3] + 1) & 7u) << 9) | (((uint32_t)(a[4] + 1) & 7u) << 12) | (((uint32_t)(a[5] + 1) & 15u) << 15) |
           (((uint32_t)(a[6] + 1) & 127u) << 19);
}
DEV void unpackFwd(uint32_t w, int32_t a[7]) {
    a[0] = (int32_t)(w & 7u);
    a[1] = (int32_t)((w >> 3) & 7u) - 1;
    a[2] = (int32_t)((w >> 6) & 7u) - 1;
    a[3] = (int32_t)((w >> 9) & 7u) - 1;
    a[4] = (int32_t)((w >> 12) & 7u) - 1;
    a[5] = (int32_t)((w >> 15) & 15u) - 1;
    a[6] = (int32_t)((w >> 19) & 127u) - 1;
}
// One sight disk (dx^2 + dy^2 <= sr^2) ORed into per-row bitmaps of a W-wide map ((W + 31) / 32 words a
// row): one atomicOr per covered row word.  dlo / dhi: the unit-type table's half-widths for sr <= 15
// (host-computed, DevUtt::diskLo/Hi); a larger sight takes the integer square root per row.
DEV void paintDiskRows(uint32_t* rows, int H, int W, int x, int y, int sr, uint32_t dlo, uint32_t dhi) {
    const int WPR = (W + 31) >> 5;
    for (int dy = -sr; dy <= sr; dy++) {
        const int yy = y + dy;
        if (yy < 0 || yy >= H) continue;
        const int ady = dy < 0 ? -dy : dy;
        int w;
        if (sr <= 15) {
            w = (int)(((ady < 8 ? dlo : dhi) >> (4 * (ady & 7))) & 0xFu);
        } else {
            const int lim = sr * sr - dy * dy;
            w = (int)__builtin_sqrtf((float)lim);
            while (w * w > lim) w--;
            while ((w + 1) * (w + 1) <= lim) w++;
        }
        const int x0 = max(0, x - w), x1 = min(W - 1, x + w);
        for (int k = x0 >> 5; k <= (x1 >> 5); k++) {
            const int lo = max(x0, 32 * k) - 32 * k, hi = min(x1, 32 * k + 31) - 32 * k;
            const uint32_t b = (hi - lo == 31) ? 0xFFFFFFFFu : (((1u << (hi - lo + 1)) - 1u) << lo);
            atomicOr(&rows[yy * WPR + k], b);
        }
    }
}
// nw words of a chunk to global memory as dwordx4 where whole vectors lie inside it: LDS word t <-> gp[t], the
// chunk at t in [a, a + nw) with gp 16-byte aligned (a = the chunk's word offset in its vector).  lds null: zeros.
// nl: the lanes that call it (lane in [0, nl)).
DEV void headFlush(const int32_t* lds, int32_t* gp, int a, int nw, int lane, int nl = 64) {
    const int nv = (a + nw + 3) >> 2;
    for (int v = lane; v < nv; v += nl) {
        const int t = 4 * v;
        const int4 x = lds ? ((const int4*)lds)[v] : make_int4(0, 0, 0, 0);
        if (t >= a && t + 4 <= a + nw) {
            ((int4*)gp)[v] = x;
        } else {
            const int xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (t + k >= a && t + k < a + nw) gp[t + k] = xs[k];
        }
    }
}
// nh halfwords of a chunk: LDS halfword t <-> gp[t], the chunk at t in [a, a + nh) with gp 16-byte aligned (a = the
// chunk's halfword offset 0..7 in its vector).  Whole vectors inside the chunk leave as dwordx4, the edges as 16-bit
// stores — never a dword: the halfword next to an edge is another wave's, or lies past the tensor.  lds null: zeros.
DEV void headFlush(const uint16_t* lds, uint16_t* gp, int a, int nh, int lane, int nl = 64) {
    const int nv = (a + nh + 7) >> 3;
    for (int v = lane; v < nv; v += nl) {
        const int t = 8 * v;
        const int4 x = lds ? ((const int4*)lds)[v] : make_int4(0, 0, 0, 0);
        if (t >= a && t + 8 <= a + nh) {
            ((int4*)gp)[v] = x;
        } else {
            const int xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (int k = 0; k < 8; k++)
                if (t + k >= a && t + k < a + nh) gp[t + k] = (uint16_t)((uint32_t)xs[k >> 1] >> (16 * (k & 1)));
        }
    }
}
// nb bytes of a chunk to global memory as dwordx4 where whole vectors lie inside it: LDS byte t <-> gp[t], the chunk
// at t in [a, a + nb) with gp 16-byte aligned.  lds null: zeros.
DEV void headFlushBytes(const uint8_t* lds, uint8_t* gp, int a, int nb, int lane, int nl = 64) {
    const int nv = (a + nb + 15) >> 4;
    for (int v = lane; v < nv; v += nl) {
        const int t = 16 * v;
        if (t >= a && t + 16 <= a + nb) {
            ((int4*)gp)[v] = lds ? ((const int4*)lds)[v] : make_int4(0, 0, 0, 0);
        } else {
            for (int k = 0; k < 16; k++)
                if (t + k >= a && t + k < a + nb) gp[t + k] = lds ? lds[t + k] : (uint8_t)0;
        }
    }
}
}  // namespace

#ifdef MRTS_LANE_AUDIT
// this unit's record into out[256] (a slot another unit filled stays unless this one has a violation there)
template <>
hipError_t mrts::laneAuditUnit<MRTS_UNIT>(int32_t* out, int reset) {
    int32_t h[256] = {};
    hipError_t e = hipMemcpyFromSymbol(h, HIP_SYMBOL(g_laneAudit), sizeof(h));
    for (int i = 0; i < 256; i++)
        if (h[i]) out[i] = h[i];
    if (e == hipSuccess && reset) {
        const int32_t z[256] = {};
        e = hipMemcpyToSymbol(HIP_SYMBOL(g_laneAudit), z, sizeof(z));
    }
    return e;
}
#endif
