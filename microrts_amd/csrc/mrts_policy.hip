// mrts_policy.hip — gfx950 kernels that choose actions: the masked-uniform and the unmasked uniform random policies
// (the bench / rollout agents) and the masked policy head (sample, score, differentiate; plain and packed rows).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#define MRTS_UNIT 1
#include "mrts_device.h"

namespace {

// ---------------------------------------------------------------- random policy (bench / rollouts)
DEV void sampleBits(const PolicyParams& Q, uint64_t lo, uint64_t hi, int slot, int c, int32_t a[7]) {
    sampleBitsRaw(Q.seed, Q.step, Q.slot_id_base + (uint32_t)slot, Q.ntypes, Q.K, lo, hi, c, a);
}
DEV void sampleCell(const PolicyParams& Q, const uint8_t* m, int slot, int c, int32_t a[7]) {
    for (int k = 0; k < 7; k++) a[k] = 0;
    if (!m[0]) return;
    uint64_t lo = 0, hi = 0;
    for (int i = 1; i < Q.K; i++) {
        const uint64_t b = m[i] ? 1ull : 0ull;
        if (i - 1 < 64) lo |= b << (i - 1);
        else hi |= b << (i - 1 - 64);
    }
    sampleBits(Q, lo, hi, slot, c, a);
}
// 16 mask bytes (0 / non-zero) -> 16 bits, byte k -> bit k
DEV uint32_t nz4(uint32_t w) {
    uint32_t t = w | (w >> 4);
    t |= t >> 2;
    t |= t >> 1;
    return ((t & 0x01010101u) * 0x01020408u) >> 24;
}
DEV uint32_t pack16(uint4 v) { return nz4(v.x) | (nz4(v.y) << 4) | (nz4(v.z) << 8) | (nz4(v.w) << 12); }

// Tiled form: one wave = 64 cells of one slot.  The 64 mask records (64*K bytes, 16-B aligned when
// HW*K and 64*K are multiples of 16) stream in with dwordx4 loads and are packed to bits in
// registers on arrival (LDS holds 1 bit per mask byte); the 64 action rows (1792 B) stream out of
// LDS with dwordx4 stores.
__global__ __launch_bounds__(64) void k_policy_tiled(PolicyParams Q) {
    __shared__ uint16_t tb[64 * 96 / 16 + 8];
    __shared__ __align__(16) int32_t sa[64 * 7];
    const int lane = (int)threadIdx.x, slot = (int)blockIdx.y;
    const int c0 = (int)blockIdx.x * 64;
    const int ncell = min(64, Q.HW - c0);
    const uint8_t* src = Q.masks + ((size_t)slot * Q.HW + c0) * Q.K;
    const int nbytes = ncell * Q.K, n16 = nbytes >> 4;
    for (int i = lane; i < n16; i += 64) tb[i] = (uint16_t)pack16(((const uint4*)src)[i]);
    if (lane == 0 && (nbytes & 15)) {
        uint32_t b = 0;
        for (int i = 16 * n16; i < nbytes; i++) b |= (src[i] ? 1u : 0u) << (i - 16 * n16);
        tb[n16] = (uint16_t)b;
    }
    __syncthreads();
    int32_t a[7] = {0, 0, 0, 0, 0, 0, 0};
    if (lane < ncell) {
        const int b0 = lane * Q.K;
        if ((tb[b0 >> 4] >> (b0 & 15)) & 1) {
            // bits b0+1 .. b0+K-1 -> lo/hi
            const int s = b0 + 1, w0 = s >> 4, sh = s & 15;
            uint64_t x0 = 0, x1 = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) x0 |= (uint64_t)tb[w0 + j] << (16 * j);
#pragma unroll
            for (int j = 0; j < 3; j++) x1 |= (uint64_t)tb[w0 + 4 + j] << (16 * j);
            uint64_t lo = sh ? ((x0 >> sh) | (x1 << (64 - sh))) : x0;
            uint64_t hi = x1 >> sh;
            const int nb = Q.K - 1;  // valid bits
            if (nb < 64) {
                lo &= (1ull << nb) - 1;
                hi = 0;
            } else if (nb < 128) {
                hi &= (1ull << (nb - 64)) - 1;
            }
            sampleBits(Q, lo, hi, slot, c0 + lane, a);
        }
    }
#pragma unroll
    for (int k = 0; k < 7; k++) sa[lane * 7 + k] = a[k];
    __syncthreads();
    int32_t* dst = Q.actions + ((size_t)slot * Q.HW + c0) * 7;
    const int nw = ncell * 7, nw4 = nw >> 2;
    for (int i = lane; i < nw4; i += 64) ((int4*)dst)[i] = ((const int4*)sa)[i];
    for (int i = 4 * nw4 + lane; i < nw; i += 64) dst[i] = sa[i];
}

// one candidate cell's action from its K-byte mask record: record bits 0..K-1 gathered from the
// covering aligned 16-B chunks (chunk q's byte 0 sits at record bit pos = 16q - b0)
DEV void sampleRecord(const PolicyParams& Q, const uint8_t* mrec, int slot, int c, int32_t row[7]) {
    const int b0 = c * Q.K, j0 = b0 >> 4, j1 = (b0 + Q.K - 1) >> 4;
    uint64_t r0 = 0, r1 = 0;
    for (int q = j0; q <= j1; q++) {
        const uint64_t b16 = pack16(((const uint4*)mrec)[q]);
        const int pos = 16 * q - b0;
        if (pos < 0) {
            r0 |= b16 >> (-pos);
        } else if (pos < 64) {
            r0 |= b16 << pos;
            if (pos > 48) r1 |= b16 >> (64 - pos);
        } else {
            r1 |= b16 << (pos - 64);
        }
    }
    // record bits 1..K-1 -> lo/hi (bit i -> bit i-1)
    uint64_t lo = (r0 >> 1) | (r1 << 63), hi = r1 >> 1;
    const int nb = Q.K - 1;
    if (nb < 64) {
        lo &= (1ull << nb) - 1;
        hi = 0;
    } else {
        hi &= (1ull << (nb - 64)) - 1;
    }
    sampleBits(Q, lo, hi, slot, c, row);
}

// Source-bit form: one wave = one slot.  Candidate cells come from the env's source bits; only their
// mask records are read (the <= 6 aligned 16-B chunks covering each).  Rows are composed in LDS,
// 256 cells (7 KB) at a time, and leave with coalesced dwordx4 stores.
__global__ __launch_bounds__(64) void k_policy_src(PolicyParams Q) {
    __shared__ __align__(16) int32_t sa[256 * 7];
    const int lane = (int)threadIdx.x, slot = (int)blockIdx.x;
    const int MW = (Q.HW + 31) / 32;
    const uint32_t* src = Q.source + (size_t)slot * MW;
    const uint8_t* mrec = Q.masks + (size_t)slot * Q.HW * Q.K;
    int32_t* dst = Q.actions + (size_t)slot * Q.HW * 7;
    for (int c0 = 0; c0 < Q.HW; c0 += 256) {
        const int ncell = min(256, Q.HW - c0);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int c = c0 + 64 * j + lane;
            int32_t row[7] = {0, 0, 0, 0, 0, 0, 0};
            if (c < Q.HW && ((src[c >> 5] >> (c & 31)) & 1u)) sampleRecord(Q, mrec, slot, c, row);
            const int r = 64 * j + lane;  // stride-7 words: conflict-free LDS writes
#pragma unroll
            for (int k = 0; k < 7; k++) sa[r * 7 + k] = row[k];
        }
        __syncthreads();
        int32_t* d = dst + (size_t)c0 * 7;
        const int nw = ncell * 7, nw4 = nw >> 2;
        for (int i = lane; i < nw4; i += 64) ((int4*)d)[i] = ((const int4*)sa)[i];
        for (int i = 4 * nw4 + lane; i < nw; i += 64) d[i] = sa[i];
        __syncthreads();
    }
    if (Q.prev_out)
        for (int w = lane; w < MW; w += 64) Q.prev_out[(size_t)slot * MW + w] = src[w];
}

// Delta form (actions holds this policy's previous output, whose candidate set is prev): only rows
// in prev | source change — candidates get a fresh action, former candidates a zero row.  A wave
// takes 64 (slot, 32-cell bit word) items in one load round, compacts their dirty cells into an LDS
// list (wave prefix sum), and spreads the list over its lanes, so each dirty row costs one record
// round trip in parallel with the others.  The candidate set is double-buffered (prev -> prev_out).
__global__ __launch_bounds__(64) void k_policy_delta(PolicyParams Q) {
    __shared__ uint32_t list[64 * 32];
    const int lane = (int)threadIdx.x;
    const uint32_t MW = (uint32_t)(Q.HW + 31) / 32;
    const uint32_t nitems = (uint32_t)Q.n_slots * MW;
    const uint32_t item = blockIdx.x * 64u + (uint32_t)lane;
    const bool valid = item < nitems;
    const uint32_t cur = valid ? Q.source[item] : 0u, old = valid ? Q.prev[item] : 0u;
    if (valid) Q.prev_out[item] = cur;
    const uint32_t dirty = cur | old;
    const int n = __popc(dirty);
    const int incl = wave_incl_sum(n);  // inclusive prefix sum over lanes
    const int total = rl(incl, 63);
    if (total == 0) return;
    const uint32_t slot = item / MW, w = item - slot * MW;
    int k = incl - n;
    for (uint32_t d = dirty; d; d &= d - 1) {
        const int b = __builtin_ctz(d);
        // row index slot*HW + cell (< 2^31 by the host's size checks), bit 31 = candidate
        list[k++] = (slot * (uint32_t)Q.HW + 32u * w + (uint32_t)b) | (((cur >> b) & 1u) << 31);
    }
    __syncthreads();
    for (int i = lane; i < total; i += 64) {
        const uint32_t e = list[i], r = e & 0x7FFFFFFFu;
        const int sl = (int)(r / (uint32_t)Q.HW), c = (int)(r - (uint32_t)sl * Q.HW);
        int32_t row[7] = {0, 0, 0, 0, 0, 0, 0};
        if (e >> 31) sampleRecord(Q, Q.masks + (size_t)sl * Q.HW * Q.K, sl, c, row);
        int32_t* dst = Q.actions + (size_t)r * 7;
#pragma unroll
        for (int q = 0; q < 7; q++) dst[q] = row[q];
    }
}

__global__ __launch_bounds__(64) void k_policy(PolicyParams Q) {
    const int c = (int)(blockIdx.x * 64 + threadIdx.x);
    const int slot = (int)blockIdx.y;
    if (c >= Q.HW) return;
    int32_t a[7];
    sampleCell(Q, Q.masks + ((size_t)slot * Q.HW + c) * Q.K, slot, c, a);
    int32_t* out = Q.actions + ((size_t)slot * Q.HW + c) * 7;
#pragma unroll
    for (int k = 0; k < 7; k++) out[k] = a[k];
}

// ---------------------------------------------------------------- masked policy head
// Logits [rows][HW][K-1] (logit j <-> mask slot j + 1) -> per candidate cell (mask slot 0) one independent masked
// categorical per non-empty field: type [0,6), the four directions [6,22), produce type [22,22+ntypes), attack
// window [22+ntypes,K-1).  One wave per row; a candidate cell is worked by a 16-lane DPP row, four cells at a
// time.  A lane owns one logit of the type field, one of the 16 direction logits (a field per quad), one produce
// type and four consecutive attack-window logits, so every field is one quad or one row and its maximum, sums
// and running sum are DPP operations inside it.
constexpr uint32_t HEAD_TAG = 0x48454144u;  // "HEAD": Philox counter word 3 (and HEAD_TAG + 1), apart from 0 / UNIFORM_TAG

// The logits' element type E (HEAD_LT_*): float, or one of the two 16-bit types.  A 16-bit logit becomes fp32 exactly at
// its load (a 16-bit load: with an odd K - 1 a cell's row is only 2-byte aligned) and every step after that is the
// float instance's; a gradient element is the float instance's value rounded once, to nearest even, at its LDS store.
struct Bf16 {
    uint16_t v;
};
struct F16 {
    _Float16 v;
};
DEV float headLoad(const float* p, int j) { return p[j]; }
DEV float headLoad(const Bf16* p, int j) { return __uint_as_float((uint32_t)p[j].v << 16); }
// v_cvt_f32_f16: exact, subnormals included (fp16 denormals are on in the default float mode, and this unit is
// compiled with it)
DEV float headLoad(const F16* p, int j) { return (float)p[j].v; }
DEV void headStore(float* p, float v) { *p = v; }
// integer round to nearest even, a NaN to the quiet NaN: what torch's float -> bfloat16 cast does
DEV void headStore(Bf16* p, float v) {
    const uint32_t u = __float_as_uint(v);
    p->v = v != v ? (uint16_t)0x7FC0u : (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
DEV void headStore(F16* p, float v) { p->v = (_Float16)v; }  // v_cvt_f16_f32 in the default mode: nearest even, subnormals kept
template <typename E>
DEV E headNaN();
template <>
DEV float headNaN<float>() { return __int_as_float(0x7FC00000); }
template <>
DEV Bf16 headNaN<Bf16>() { return Bf16{(uint16_t)0x7FC0u}; }
template <>
DEV F16 headNaN<F16>() { return F16{__builtin_bit_cast(_Float16, (uint16_t)0x7E00u)}; }
// what a chunk of E leaves through (headFlush): words for float, halfwords for the 16-bit types
template <typename E>
struct HeadOut {
    using T = int32_t;
    static constexpr int LG = 2;  // log2 of the elements per 16-byte vector
};
template <>
struct HeadOut<Bf16> {
    using T = uint16_t;
    static constexpr int LG = 3;
};
template <>
struct HeadOut<F16> : HeadOut<Bf16> {};

template <int CTRL, int ROWS = 0xF>
DEV float dppF(float old, float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), CTRL, ROWS, 0xF, false));
}
// max / sum over each W-lane segment (a quad or a 16-lane row), the result on every lane of it: each step
// combines two values that are already equal across the lanes they came from, so the lanes agree bit for bit
template <int W>
DEV float segMax(float v) {
    LANE_AUDIT_WAVE(2);
    v = fmaxf(v, dppF<0xB1>(v, v));  // quad_perm [1,0,3,2]
    v = fmaxf(v, dppF<0x4E>(v, v));  // quad_perm [2,3,0,1]
    if (W == 16) {
        v = fmaxf(v, dppF<0x141>(v, v));  // row_half_mirror
        v = fmaxf(v, dppF<0x140>(v, v));  // row_mirror
    }
    return v;
}
template <int W>
DEV float segSum(float v) {
    LANE_AUDIT_WAVE(2);
    v += dppF<0xB1>(v, v);
    v += dppF<0x4E>(v, v);
    if (W == 16) {
        v += dppF<0x141>(v, v);
        v += dppF<0x140>(v, v);
    }
    return v;
}
// inclusive running sum over each segment, in lane order (ql: the lane's index in its segment)
template <int W>
DEV float segScan(float v, int ql) {
    LANE_AUDIT_WAVE(2);
    if (W == 16) {
        v += dppF<0x111>(0.f, v);  // row_shr:1 (lanes shifted in from outside the row read 0)
        v += dppF<0x112>(0.f, v);
        v += dppF<0x114>(0.f, v);
        v += dppF<0x118>(0.f, v);
    } else {
        const float t1 = dppF<0x90>(0.f, v);  // quad_perm [0,0,1,2]
        v += ql >= 1 ? t1 : 0.f;
        const float t2 = dppF<0x40>(0.f, v);  // quad_perm [0,0,0,1]
        v += ql >= 2 ? t2 : 0.f;
    }
    return v;
}
// a double through DPP as its two halves (lanes without a source read 0.0)
template <int CTRL, int ROWS = 0xF>
DEV double dppD(double v) {
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)b, CTRL, ROWS, 0xF, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(b >> 32), CTRL, ROWS, 0xF, false);
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}
// sum over the wave in a fixed order (wave_reduce's DPP chain on doubles): a row's log-probability and entropy add
// up to 64 x 7 fp32 terms per lane, and double partial sums keep their rounding below that of the terms
DEV double waveSumD(double v) {
    LANE_AUDIT_WAVE(2);
    v += dppD<0xB1>(v);
    v += dppD<0x4E>(v);
    v += dppD<0x141>(v);
    v += dppD<0x140>(v);
    v += dppD<0x142, 0xA>(v);
    v += dppD<0x143, 0xC>(v);
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)rl((int)(uint32_t)b, 63), hi = (uint32_t)rl((int)(uint32_t)(b >> 32), 63);
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

// one candidate cell as its 16-lane row sees it (E: the logits' element type)
template <typename E>
struct HeadCell {
    bool act;             // the row has a cell this round
    const E* lrow;        // its K-1 logits
    const uint8_t* mrec;  // its K mask bytes
    const int32_t* arow;  // SCORE / GRAD: its given action row
    int32_t* srow;        // SAMPLE: its action row in LDS (zeroed)
    E* grow;              // GRAD: its gradient row in LDS (zeroed)
    float glp, gent;      // GRAD: the row's upstream gradients
    double lp, ent;       // per-lane partial sums of the row's log-probability and entropy (fp32 terms)
    uint32_t w0, wd, w5, w6;  // SAMPLE: the Philox words of the lane's fields (type, its direction field, produce type, attack)
};

// One field, NE logits per lane (l / set: the lane's logits and mask bits, 0 / false outside the field), the field
// spanning a W-lane segment.  idx0: the field-local index of l[0]; a: the given component (SCORE / GRAD).
template <int MODE, int NE, int W, typename E>
DEV void headField(HeadCell<E>& X, int lane, const float* l, const bool* set, int j0, int idx0, int field, uint32_t word, int a) {
#pragma clang fp contract(off)
    const int ql = lane & (W - 1), segbase = lane - ql;
    const uint32_t segmask = (1u << W) - 1u;
    float mx = -INFINITY;
    bool anyset = false;
#pragma unroll
    for (int k = 0; k < NE; k++) {
        mx = set[k] ? fmaxf(mx, l[k]) : mx;
        anyset |= set[k];
    }
    mx = segMax<W>(mx);
    const uint32_t sb = (uint32_t)(ballot(anyset) >> segbase) & segmask;
    const bool nonempty = sb != 0;
    float e[NE], lt = 0.f, tt = 0.f;
#pragma unroll
    for (int k = 0; k < NE; k++) {
        const float d = l[k] - mx;
        e[k] = set[k] ? expf(d) : 0.f;
        lt += e[k];
        tt += set[k] ? e[k] * d : 0.f;
    }
    const float S = segSum<W>(lt), T = segSum<W>(tt);
    const float logS = logf(S), H = logS - T / S;
    X.ent += (nonempty && ql == 0) ? (double)H : 0.0;
    if (MODE == HEAD_SAMPLE) {
        // the smallest set bit whose running sum exceeds u * S, else (rounding) the last set bit
        const float thr = (float)(word >> 8) * 0x1p-24f * S;
        float run = segScan<W>(lt, ql);
        if (NE > 1) run = dppF<0x111>(0.f, run);  // exclusive: the lanes before this one
        bool hit[NE], anyhit = false;
#pragma unroll
        for (int k = 0; k < NE; k++) {
            if (NE > 1) run += e[k];
            hit[k] = set[k] && run > thr;
            anyhit |= hit[k];
        }
        const uint32_t hb = (uint32_t)(ballot(anyhit) >> segbase) & segmask;
        const int pick = hb ? __builtin_ctz(hb) : (sb ? 31 - __builtin_clz(sb) : 0);
        int kk = -1;
        float dsel = 0.f;
#pragma unroll
        for (int k = NE - 1; k >= 0; k--)
            if (hit[k]) {
                kk = k;
                dsel = l[k] - mx;
            }
        if (kk < 0) {
#pragma unroll
            for (int k = 0; k < NE; k++)
                if (set[k]) {
                    kk = k;
                    dsel = l[k] - mx;
                }
        }
        if (nonempty && ql == pick) {
            X.srow[field] = idx0 + kk;
            X.lp += (double)(dsel - logS);
        }
    } else {
        bool match[NE], anym = false;
#pragma unroll
        for (int k = 0; k < NE; k++) {
            match[k] = set[k] && idx0 + k == a;
            anym |= match[k];
        }
        const bool hasA = ((uint32_t)(ballot(anym) >> segbase) & segmask) != 0;
        if (MODE == HEAD_SCORE) {
#pragma unroll
            for (int k = 0; k < NE; k++) X.lp += match[k] ? (double)((l[k] - mx) - logS) : 0.0;
            // a component outside the field's set bits: the row's log-probability is -inf
            X.lp += (nonempty && !hasA && ql == 0) ? (double)-INFINITY : 0.0;
        } else {
#pragma unroll
            for (int k = 0; k < NE; k++)
                if (set[k]) {
                    const float p = e[k] / S, logp = (l[k] - mx) - logS;
                    float gv = X.gent * (-p * (logp + H));
                    if (hasA) gv += X.glp * ((match[k] ? 1.f : 0.f) - p);
                    headStore(X.grow + j0 + k, gv);
                }
        }
    }
}

template <int MODE, typename E>
DEV void headCell(HeadCell<E>& X, const HeadParams& Q, int lane) {
    const int q = lane & 15, nt = Q.ntypes, natt = Q.K - 23 - nt;
    // the lane's seven logits: 0 type, 1 a direction (quad = field), 2 produce type, 3..6 attack window 4q..4q+3
    int j[7];
    bool in[7];
    j[0] = q, in[0] = q < 6;
    j[1] = 6 + q, in[1] = true;
    j[2] = 22 + q, in[2] = q < nt;
#pragma unroll
    for (int k = 0; k < 4; k++) j[3 + k] = 22 + nt + 4 * q + k, in[3 + k] = 4 * q + k < natt;
    // Unconditional loads (a lane without a logit of the field, or a row without a cell this round, reads logit 0
    // of a cell of the chunk): all fourteen are in flight together, one memory round per cell.  The logit of a
    // cleared bit comes with its row's cache lines and is dropped by the select: it never reaches the arithmetic.
    float l[7];
    bool set[7];
#pragma unroll
    for (int i = 0; i < 7; i++) {
        const int jj = in[i] ? j[i] : 0;
        const uint32_t mb = X.mrec[1 + jj];
        const float lv = headLoad(X.lrow, jj);
        set[i] = X.act && in[i] && mb != 0;
        l[i] = set[i] ? lv : 0.f;
    }
    const int dq = q >> 2;
    int a0 = 0, a1 = 0, a5 = 0, a6 = 0;
    if (MODE != HEAD_SAMPLE && X.act) a0 = X.arow[0], a1 = X.arow[1 + dq], a5 = X.arow[5], a6 = X.arow[6];
    headField<MODE, 1, 16>(X, lane, l + 0, set + 0, j[0], q, 0, X.w0, a0);
    headField<MODE, 1, 4>(X, lane, l + 1, set + 1, j[1], q & 3, 1 + dq, X.wd, a1);
    headField<MODE, 1, 16>(X, lane, l + 2, set + 2, j[2], q, 5, X.w5, a5);
    headField<MODE, 4, 16>(X, lane, l + 3, set + 3, j[3], 4 * q, 6, X.w6, a6);
}

// One wave per row.  Per 64 cells: the candidate bits (source bits, or mask byte 0) as one ballot; SAMPLE / GRAD
// compose the chunk's action / gradient rows in zeroed LDS and store them with dwordx4, a chunk without a
// candidate as plain zero stores.  The row's log-probability and entropy are per-lane partial sums added up by one
// DPP chain at the end: a fixed order, no atomics.
template <int MODE, typename E>
__global__ __launch_bounds__(64) void k_head(HeadParams Q) {
    // what this mode writes: action rows as words, gradient rows as elements of E (words for float); LG: log2 of the
    // elements per 16-byte vector
    using O = typename std::conditional<MODE == HEAD_GRAD, typename HeadOut<E>::T, int32_t>::type;
    constexpr int LG = MODE == HEAD_GRAD ? HeadOut<E>::LG : 2;
    __shared__ __align__(16) int32_t sbuf[(MODE == HEAD_GRAD ? 64 * HEAD_MAX_LOGITS * (int)sizeof(O) / 4 : MODE == HEAD_SAMPLE ? 64 * 7 : 0) + 8];
    const int lane = (int)threadIdx.x, row = (int)blockIdx.x, KL = Q.K - 1;
    const int RW = MODE == HEAD_GRAD ? KL : 7;  // elements per cell of what this mode writes
    const size_t cell0 = (size_t)row * Q.HW;
    const uint32_t* src = (MODE == HEAD_SAMPLE && Q.source) ? Q.source + (size_t)row * ((Q.HW + 31) / 32) : nullptr;
    O* out = MODE == HEAD_GRAD ? (O*)Q.grad : (O*)Q.actions;
    HeadCell<E> X;
    X.lp = X.ent = 0.0;
    X.glp = X.gent = 0.f;
    if (MODE == HEAD_GRAD) {
        if (Q.g_logprob) X.glp = Q.g_logprob[row];
        if (Q.g_entropy) X.gent = Q.g_entropy[row];
    }
    for (int c0 = 0; c0 < Q.HW; c0 += 64) {
        const int ncell = min(64, Q.HW - c0), c = c0 + lane;
        bool cand = false;
        if (c < Q.HW) cand = src ? ((src[c >> 5] >> (c & 31)) & 1u) != 0 : Q.masks[(cell0 + c) * Q.K] != 0;
        uint64_t m = ballot(cand);
        O* gp = nullptr;
        int a = 0, nw = 0;
        if (MODE != HEAD_SCORE) {
            O* p = out + (cell0 + c0) * RW;
            a = (int)(((uintptr_t)p / sizeof(O)) & ((1 << LG) - 1));
            gp = p - a;
            nw = ncell * RW;
            if (m == 0) {
                headFlush((const O*)nullptr, gp, a, nw, lane);
                continue;
            }
            for (int v = lane; v < ((a + nw + (1 << LG) - 1) >> LG); v += 64) ((int4*)sbuf)[v] = make_int4(0, 0, 0, 0);
            __syncthreads();
        } else if (m == 0) {
            continue;
        }
        while (m) {  // four candidate cells per round, the g-th to row g
            int cl = -1;
#pragma unroll
            for (int g = 0; g < 4; g++)
                if (m) {
                    const int b = __builtin_ctzll(m);
                    m &= m - 1;
                    cl = (lane >> 4) == g ? b : cl;
                }
            X.act = cl >= 0;
            const size_t cell = cell0 + c0 + (cl >= 0 ? cl : 0);
            X.lrow = (const E*)Q.logits + cell * KL;
            X.mrec = Q.masks + cell * Q.K;
            X.arow = Q.actions + cell * 7;
            X.srow = sbuf + a + (cl >= 0 ? cl : 0) * 7;
            X.grow = (E*)sbuf + a + (cl >= 0 ? cl : 0) * KL;
            if (MODE == HEAD_SAMPLE) {
                const uint32_t sid = Q.slot_id_base + (uint32_t)row, cc = (uint32_t)(c0 + (cl >= 0 ? cl : 0));
                uint32_t c1[4] = {sid, Q.step, cc, HEAD_TAG}, c2[4] = {sid, Q.step, cc, HEAD_TAG + 1u};
                philox(c1, (uint32_t)Q.seed, (uint32_t)(Q.seed >> 32));
                philox(c2, (uint32_t)Q.seed, (uint32_t)(Q.seed >> 32));
                // eight words, field f's uniform from word f; the lane's direction field is 1 + its quad
                const uint32_t p1 = c1[1], p2 = c1[2], p3 = c1[3], p4 = c2[0];
                const int dq = (lane >> 2) & 3;
                X.w0 = c1[0];
                X.wd = dq == 0 ? p1 : dq == 1 ? p2 : dq == 2 ? p3 : p4;
                X.w5 = c2[1];
                X.w6 = c2[2];
            }
            headCell<MODE>(X, Q, lane);
        }
        if (MODE != HEAD_SCORE) {
            __syncthreads();
            headFlush((const O*)sbuf, gp, a, nw, lane);
            __syncthreads();
        }
    }
    if (MODE != HEAD_GRAD) {
        const float lp = (float)waveSumD(X.lp), ent = (float)waveSumD(X.ent);
        if (lane == 0) {
            if (Q.logprob) Q.logprob[row] = lp;
            if (Q.entropy) Q.entropy[row] = ent;
        }
    }
}

// ---- Packed policy rows (include/mrts.h): the candidates of a row as HEAD_CW words each, for rollout storage ----
// an action component's code: itself inside [0, off), else off (off = all ones of the component's bits, beyond
// every field's width: a component the dense score finds outside its field's set bits stays outside them)
DEV uint32_t headActWord(const int32_t* a) {
    uint32_t w = 0;
#pragma unroll
    for (int f = 0; f < 7; f++) {
        const uint32_t off = (1u << HEAD_ACT_BITS[f]) - 1u, v = (uint32_t)a[f];
        w |= (v < off ? v : off) << HEAD_ACT_SHIFT[f];
    }
    return w;
}
DEV int32_t headActComp(uint32_t w, int f) {
    int sh = 0, bits = 0;
#pragma unroll
    for (int k = 0; k < 7; k++)
        if (k == f) sh = HEAD_ACT_SHIFT[k], bits = HEAD_ACT_BITS[k];
    const uint32_t off = (1u << bits) - 1u, v = (w >> sh) & off;
    return v == off ? -1 : (int32_t)v;
}
// four mask bits as four 0 / 1 bytes
DEV uint32_t headSpread4(uint32_t b) { return (b & 1u) | ((b & 2u) << 7) | ((b & 4u) << 14) | ((b & 8u) << 21); }
DEV uint32_t headBits4(uint32_t b0, uint32_t b1, uint32_t b2, int w) {  // bits 4w..4w+3 of the 96
    const uint32_t x = w < 8 ? b0 : w < 16 ? b1 : b2;
    return (x >> (4 * (w & 7))) & 15u;
}
// the packed row a block works: packed row index[row] (row without an index); ok false when that is out of range
DEV const uint32_t* headPackedRow(const HeadPackedParams& P, int row, bool& ok) {
    const int64_t pr = P.index ? (int64_t)P.index[row] : (int64_t)row;
    ok = pr >= 0 && pr < (int64_t)P.n_packed;
    return P.packed + (size_t)(ok ? pr : 0) * (size_t)P.words;
}
constexpr int HEAD_STG = 128;  // candidates k_head_pack stages in LDS between flushes (a chunk adds at most 64)

// One wave per row.  Per 64 cells the candidate bits (source bits, or mask byte 0) as one ballot, as k_head finds
// them; a candidate's slot in the row is the count before its chunk plus the candidates below its lane.  The
// candidate's own lane adds its cell and action word, the wave reads its mask record (two bytes per lane) and two
// ballots give the bits.  The row is composed in LDS and stored with dwordx4 (headFlush), count word and zero tail
// included; a row of more than HEAD_STG candidates flushes in between.
__global__ __launch_bounds__(64) void k_head_pack(HeadPackedParams P) {
    __shared__ __align__(16) int32_t stg[4 + 1 + HEAD_STG * HEAD_CW + 3];
    const HeadParams& Q = P.H;
    const int lane = (int)threadIdx.x, row = (int)blockIdx.x;
    const size_t cell0 = (size_t)row * Q.HW;
    const uint32_t* src = Q.source ? Q.source + (size_t)row * ((Q.HW + 31) / 32) : nullptr;
    int32_t* orow = (int32_t*)P.packed_out + (size_t)row * (size_t)P.words;
    // staged: the row's words [r0, r0 + rn) at stg[a + (word - r0)], orow + r0 - a 16-byte aligned
    int total = 0, r0 = 0, rn = 1, a = (int)(((uintptr_t)orow >> 2) & 3);
    for (int c0 = 0; c0 < Q.HW; c0 += 64) {
        const int c = c0 + lane;
        bool cand = false;
        if (c < Q.HW) cand = src ? ((src[c >> 5] >> (c & 31)) & 1u) != 0 : Q.masks[(cell0 + c) * Q.K] != 0;
        const uint64_t m = ballot(cand);
        if (m == 0) continue;
        const int nc = __builtin_popcountll(m), keep = max(0, min(nc, P.cap - total));
        total += nc;
        if (keep == 0) continue;
        if (rn + keep * HEAD_CW > 1 + HEAD_STG * HEAD_CW) {  // word 0 waits for the count
            __syncthreads();
            if (r0 == 0) headFlush(stg, orow - a, a + 1, rn - 1, lane);
            else headFlush(stg, orow + r0 - a, a, rn, lane);
            __syncthreads();
            r0 += rn;
            rn = 0;
            a = (int)(((uintptr_t)(orow + r0) >> 2) & 3);
        }
        int32_t* s = stg + a + rn;
        const int pos = lanes_below(m);
        if (cand && pos < keep) {
            s[pos * HEAD_CW] = c;
            s[pos * HEAD_CW + 1] = (int32_t)headActWord(Q.actions + (cell0 + c) * 7);
        }
        uint64_t mm = m;
        for (int k = 0; k < keep; k++) {
            const uint8_t* rec = Q.masks + (cell0 + c0 + __builtin_ctzll(mm)) * Q.K;
            mm &= mm - 1;
            const bool v0 = lane < Q.K && rec[lane < Q.K ? lane : 0] != 0;
            const bool v1 = lane + 64 < Q.K && rec[lane + 64 < Q.K ? lane + 64 : 0] != 0;
            const uint64_t b0 = ballot(v0), b1 = ballot(v1);
            if (lane == 0) {
                s[k * HEAD_CW + 2] = (int32_t)(uint32_t)b0;
                s[k * HEAD_CW + 3] = (int32_t)(uint32_t)(b0 >> 32);
                s[k * HEAD_CW + 4] = (int32_t)(uint32_t)b1;
            }
        }
        rn += keep * HEAD_CW;
    }
    if (lane == 0) {
        if (r0 == 0) stg[a] = total;
        else orow[0] = total;
        if (total > P.cap) atomicAdd(P.overflow, 1ull);
    }
    __syncthreads();
    headFlush(stg, orow + r0 - a, a, rn, lane);
    const int t0 = r0 + rn, a2 = (int)(((uintptr_t)(orow + t0) >> 2) & 3);
    headFlush(nullptr, orow + t0 - a2, a2, P.words - t0, lane);
}

// The canonical dense form of packed rows, one wave per row: per 64 cells the chunk's mask records (0 / 1 bytes)
// and action rows composed in zeroed LDS from the row's candidates of that chunk, then stored whole — every byte of
// both outputs is written.  A count above cap gives its first cap candidates; a cell outside the map or out of
// order and an index outside the packed rows give nothing.
__global__ __launch_bounds__(64) void k_head_unpack(HeadPackedParams P) {
    __shared__ __align__(16) uint8_t smask[16 + 64 * (HEAD_MAX_LOGITS + 1) + 16];
    __shared__ __align__(16) int32_t sact[4 + 64 * 7 + 4];
    const HeadParams& Q = P.H;
    const int lane = (int)threadIdx.x, row = (int)blockIdx.x;
    const size_t cell0 = (size_t)row * Q.HW;
    bool ok;
    const uint32_t* prow = headPackedRow(P, row, ok);
    const uint32_t n = ok ? min(prow[0], (uint32_t)P.cap) : 0u;
    uint32_t i0 = 0;
    for (int c0 = 0; c0 < Q.HW; c0 += 64) {
        const int ncell = min(64, Q.HW - c0);
        uint8_t* mp = P.masks_out + (cell0 + c0) * Q.K;
        int32_t* ap = P.actions_out + (cell0 + c0) * 7;
        const int am = (int)((uintptr_t)mp & 15), aa = (int)(((uintptr_t)ap >> 2) & 3);
        const int nb = ncell * Q.K, nw = ncell * 7;
        for (int v = lane; v < ((am + nb + 15) >> 4); v += 64) ((int4*)smask)[v] = make_int4(0, 0, 0, 0);
        for (int v = lane; v < ((aa + nw + 3) >> 2); v += 64) ((int4*)sact)[v] = make_int4(0, 0, 0, 0);
        __syncthreads();
        while (i0 < n) {
            const uint32_t* cw = prow + 1 + (size_t)i0 * HEAD_CW;
            const uint32_t cell = cw[0];
            if ((cell >> 6) != (uint32_t)(c0 >> 6)) break;
            i0++;
            if (cell >= (uint32_t)Q.HW) continue;
            const int cl = (int)(cell & 63u);
            const uint32_t aw = cw[1], b0 = cw[2], b1 = cw[3], b2 = cw[4];
            if (lane < Q.K) smask[am + cl * Q.K + lane] = (uint8_t)((lane < 32 ? b0 >> lane : b1 >> (lane - 32)) & 1u);
            if (lane + 64 < Q.K) smask[am + cl * Q.K + lane + 64] = (uint8_t)((b2 >> lane) & 1u);
            if (lane < 7) sact[aa + cl * 7 + lane] = headActComp(aw, lane);
        }
        __syncthreads();
        headFlushBytes(smask, mp - am, am, nb, lane);
        headFlush(sact, ap - aa, aa, nw, lane);
        __syncthreads();
    }
}

// k_head's SCORE / GRAD on packed rows: logits row r against packed row index[r].  The rounds are k_head's — up to
// four consecutive candidates of one 64-cell chunk (cell >> 6; the row is sorted by cell), the g-th to DPP row g —
// so every lane's partial sums take the same terms in the same order and the results equal the dense kernels' bit
// for bit.  Each round expands its candidates' mask bits to 0 / 1 bytes and their action words to components in
// LDS, where headCell reads them as it reads the dense tensors.  The count and the candidate words are read at
// wave-uniform addresses inside the row (clamped to cap), so the first round's words load with the count.  A row
// whose count exceeds cap, or whose index is outside the packed rows, is NaN: logprob, entropy, gradient row.
template <int MODE, typename E>
__global__ __launch_bounds__(64) void k_head_packed(HeadPackedParams P) {
    using O = typename HeadOut<E>::T;  // the gradient rows' elements, as k_head stores them
    constexpr int LG = HeadOut<E>::LG;
    constexpr int XW = (HEAD_MAX_LOGITS + 1 + 3) / 4 + 7;  // per DPP row: the mask bytes, then the action row
    __shared__ __align__(16) int32_t sbuf[(MODE == HEAD_GRAD ? 64 * HEAD_MAX_LOGITS * (int)sizeof(O) / 4 : 0) + 8];
    __shared__ __align__(16) uint32_t sexp[4 * XW];
    const HeadParams& Q = P.H;
    const int lane = (int)threadIdx.x, row = (int)blockIdx.x, KL = Q.K - 1, g = lane >> 4, q = lane & 15;
    const size_t cell0 = (size_t)row * Q.HW;
    bool ok;
    const uint32_t* prow = headPackedRow(P, row, ok);
    const uint32_t n = prow[0], last = (uint32_t)P.cap - 1u;
    uint32_t i0 = 0, cc = prow[1];  // cc: the cell of candidate i0
    if (!ok || n > (uint32_t)P.cap) {
        const float nan = __int_as_float(0x7FC00000);
        if (MODE == HEAD_GRAD) {
            for (size_t t = lane; t < (size_t)Q.HW * KL; t += 64) ((E*)Q.grad)[cell0 * KL + t] = headNaN<E>();
        } else if (lane == 0) {
            if (Q.logprob) Q.logprob[row] = nan;
            if (Q.entropy) Q.entropy[row] = nan;
        }
        return;
    }
    HeadCell<E> X;
    X.lp = X.ent = 0.0;
    X.glp = X.gent = 0.f;
    X.srow = nullptr;
    X.w0 = X.wd = X.w5 = X.w6 = 0;
    if (MODE == HEAD_GRAD) {
        if (Q.g_logprob) X.glp = Q.g_logprob[row];
        if (Q.g_entropy) X.gent = Q.g_entropy[row];
    }
    uint32_t* xr = sexp + g * XW;
    for (int c0 = 0; c0 < Q.HW; c0 += 64) {
        const uint32_t chunk = (uint32_t)(c0 >> 6);
        const bool has = i0 < n && (cc >> 6) == chunk;
        O* gp = nullptr;
        int a = 0, nw = 0;
        if (MODE == HEAD_GRAD) {
            O* p = (O*)Q.grad + (cell0 + c0) * KL;
            a = (int)(((uintptr_t)p / sizeof(O)) & ((1 << LG) - 1));
            gp = p - a;
            nw = min(64, Q.HW - c0) * KL;
            if (!has) {
                headFlush((const O*)nullptr, gp, a, nw, lane);
                continue;
            }
            for (int v = lane; v < ((a + nw + (1 << LG) - 1) >> LG); v += 64) ((int4*)sbuf)[v] = make_int4(0, 0, 0, 0);
        } else if (!has) {
            if (i0 >= n) break;
            continue;
        }
        while (i0 < n && (cc >> 6) == chunk) {  // four candidate cells per round, the g-th to row g
            uint32_t cl[5];
#pragma unroll
            for (int k = 0; k < 5; k++) cl[k] = prow[1 + (size_t)min(i0 + k, last) * HEAD_CW];
            int take = 1;
#pragma unroll
            for (int k = 1; k < 4; k++)
                if (take == k && i0 + k < n && (cl[k] >> 6) == chunk) take = k + 1;
            const uint32_t* cw = prow + 1 + (size_t)min(i0 + g, last) * HEAD_CW;
            const uint32_t cell = cw[0], aw = cw[1], b0 = cw[2], b1 = cw[3], b2 = cw[4];
            X.act = g < take && cell < (uint32_t)Q.HW;
            const uint32_t cs = X.act ? cell : 0u;
            __syncthreads();  // the previous round has read its expansion
            for (int w = q; w < (Q.K + 3) / 4; w += 16) xr[w] = headSpread4(headBits4(b0, b1, b2, w));
            if (q < 7) xr[XW - 7 + q] = (uint32_t)headActComp(aw, q);
            __syncthreads();
            X.lrow = (const E*)Q.logits + (cell0 + cs) * KL;
            X.mrec = (const uint8_t*)xr;
            X.arow = (const int32_t*)(xr + XW - 7);
            X.grow = (E*)sbuf + a + (cs & 63u) * KL;
            headCell<MODE>(X, Q, lane);
            i0 += take;
            cc = take == 1 ? cl[1] : take == 2 ? cl[2] : take == 3 ? cl[3] : cl[4];
        }
        if (MODE == HEAD_GRAD) {
            __syncthreads();
            headFlush((const O*)sbuf, gp, a, nw, lane);
            __syncthreads();
        }
    }
    if (MODE != HEAD_GRAD) {
        const float lp = (float)waveSumD(X.lp), ent = (float)waveSumD(X.ent);
        if (lane == 0) {
            if (Q.logprob) Q.logprob[row] = lp;
            if (Q.entropy) Q.entropy[row] = ent;
        }
    }
}
// the instances of one element type (the host checked ltype)
template <typename E>
void headLaunch(int mode, const HeadParams& Q, dim3 grid, dim3 block, hipStream_t stream) {
    if (mode == HEAD_SAMPLE) hipLaunchKernelGGL((k_head<HEAD_SAMPLE, E>), grid, block, 0, stream, Q);
    else if (mode == HEAD_SCORE) hipLaunchKernelGGL((k_head<HEAD_SCORE, E>), grid, block, 0, stream, Q);
    else hipLaunchKernelGGL((k_head<HEAD_GRAD, E>), grid, block, 0, stream, Q);
}
template <typename E>
void headPackedLaunch(int mode, const HeadPackedParams& P, dim3 grid, dim3 block, hipStream_t stream) {
    if (mode == HEAD_SCORE) hipLaunchKernelGGL((k_head_packed<HEAD_SCORE, E>), grid, block, 0, stream, P);
    else hipLaunchKernelGGL((k_head_packed<HEAD_GRAD, E>), grid, block, 0, stream, P);
}
}  // namespace

namespace mrts {
// Unmasked uniform random policy (BASELINE config c2), uniformRow for every cell of
// every slot.  One thread per (slot, cell): the whole action tensor, dwordx4 + dwordx3 per row.
__global__ __launch_bounds__(64) void k_policy_uniform(int32_t* __restrict__ actions, int HW, int ntypes, int natt,
                                                        uint64_t seed, uint32_t step, uint32_t slot_base) {
    const int slot = (int)blockIdx.y, c = (int)(blockIdx.x * 64 + threadIdx.x);
    if (c >= HW) return;
    int32_t a[7];
    uniformRow(seed, step, slot_base + (uint32_t)slot, c, ntypes, natt, a);
    int32_t* dst = actions + ((size_t)slot * HW + c) * 7;
    st4u<false>(dst, a[0], a[1], a[2], a[3]);
    st3u<false>(dst + 4, a[4], a[5], a[6]);
}
hipError_t launchPolicyUniform(int32_t* actions, int n_slots, int HW, int ntypes, int natt, uint64_t seed, uint32_t step,
                               uint32_t slot_base, hipStream_t stream) {
    if (n_slots <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_policy_uniform, dim3((unsigned)((HW + 63) / 64), (unsigned)n_slots), dim3(64), 0, stream, actions, HW,
                       ntypes, natt, seed, step, slot_base);
    return hipGetLastError();
}

// *prevWritten: the launch recorded its candidate set in Q.prev (a later call may use the delta form)
hipError_t launchPolicy(const PolicyParams& Q, hipStream_t stream, bool* prevWritten) {
    dim3 grid((unsigned)((Q.HW + 63) / 64), (unsigned)Q.n_slots), block(64);
    const bool srcOk = Q.source && ((size_t)Q.HW * Q.K) % 16 == 0 && Q.HW % 4 == 0 && Q.K <= 96 && Q.K >= 65;
    *prevWritten = srcOk && Q.prev_out;
    if (srcOk && Q.delta && Q.prev)
        hipLaunchKernelGGL(k_policy_delta, dim3((unsigned)(((size_t)Q.n_slots * ((Q.HW + 31) / 32) + 63) / 64)), block,
                           0, stream, Q);
    else if (srcOk)
        hipLaunchKernelGGL(k_policy_src, dim3((unsigned)Q.n_slots), block, 0, stream, Q);
    else if (((size_t)Q.HW * Q.K) % 16 == 0 && (64 * Q.K) % 16 == 0 && Q.HW % 4 == 0 && Q.K <= 96)
        hipLaunchKernelGGL(k_policy_tiled, grid, block, 0, stream, Q);
    else
        hipLaunchKernelGGL(k_policy, grid, block, 0, stream, Q);
    return hipGetLastError();
}

// mode: HEAD_SAMPLE / HEAD_SCORE / HEAD_GRAD; one 64-lane block per row (the host checked K - 1 <= HEAD_MAX_LOGITS)
hipError_t launchHead(int mode, const HeadParams& Q, hipStream_t stream) {
    if (Q.n_rows <= 0) return hipSuccess;
    const dim3 grid((unsigned)Q.n_rows), block(64);
    if (Q.ltype == HEAD_LT_F32) headLaunch<float>(mode, Q, grid, block, stream);
    else if (Q.ltype == HEAD_LT_BF16) headLaunch<Bf16>(mode, Q, grid, block, stream);
    else headLaunch<F16>(mode, Q, grid, block, stream);
    return hipGetLastError();
}

// the packed rows' kernels, one 64-lane block per row: HEAD_PACK / HEAD_UNPACK, or HEAD_SCORE / HEAD_GRAD on packed rows
hipError_t launchHeadPacked(int mode, const HeadPackedParams& P, hipStream_t stream) {
    if (P.H.n_rows <= 0) return hipSuccess;
    const dim3 grid((unsigned)P.H.n_rows), block(64);
    if (mode == HEAD_PACK) hipLaunchKernelGGL(k_head_pack, grid, block, 0, stream, P);
    else if (mode == HEAD_UNPACK) hipLaunchKernelGGL(k_head_unpack, grid, block, 0, stream, P);
    else if (P.H.ltype == HEAD_LT_F32) headPackedLaunch<float>(mode, P, grid, block, stream);
    else if (P.H.ltype == HEAD_LT_BF16) headPackedLaunch<Bf16>(mode, P, grid, block, stream);
    else headPackedLaunch<F16>(mode, P, grid, block, stream);
    return hipGetLastError();
}
}  // namespace mrts
