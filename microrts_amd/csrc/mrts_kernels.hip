// mrts_kernels.hip — gfx950 kernels for the vectorised microRTS env step.
//
// One 64-lane wavefront (= one workgroup) owns one game.  The game's units live in LDS as
// struct-of-arrays in PhysicalGameState list order (slot order == LinkedList order), with a
// cell -> slot occupancy map (one live unit per cell is an engine invariant:
// PhysicalGameState.addUnit, reference src/rts/PhysicalGameState.java:189-201).  The Java
// semantics are order-dependent (rows in cell order, fillWithNones in list order, conflict scans
// and cycle() execution in LinkedHashMap insertion order), so every ORDERED decision runs
// wave-uniformly (all lanes agree, scalar branches), while every order-free sub-problem
// (row fetch + decode, legality, conflict flags, ready ranking, death compaction, visibility,
// observation planes, legal-action masks) runs lane-parallel with ballots and DPP reductions.
// No MFMA: integer/indexing work.
// This unit is the step kernel: Game, k_env and its instances, the launch selection, the LDS sizes and the
// diagnostic builds' read-backs.  The policies are in mrts_policy.hip, the renderers in mrts_aux.hip.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#define MRTS_UNIT 0
#include "mrts_device.h"

namespace {

constexpr uint16_t EMPTY = 0xFFFF, WALL = 0xFFFE;
enum { T_NONE = 0, T_MOVE = 1, T_HARVEST = 2, T_RETURN = 3, T_PRODUCE = 4, T_ATTACK = 5 };
// (k_env's MODE_STEP .. MODE_TRACE: mrts_internal.h, shared with the host)

// Diagnostic build only (-DMRTS_PHASE_TIMING, tools/phase_timing.py): per-phase shader-clock cycles
// summed over games; not compiled into libmrts.so.
#ifdef MRTS_PHASE_TIMING
constexpr int PH_GAMES = 1 << 16;
constexpr int NPH = 32;  // phase slots
__device__ unsigned long long g_phase[NPH * PH_GAMES];  // [phase][game], no contention
__device__ unsigned long long g_span[11 * PH_GAMES];    // last launch: [game] start / end, s_memrealtime (100 MHz),
                                                       // placement: HW_ID | XCC_ID << 32 | nu at start << 40 | nu at end << 48
#ifdef MRTS_SPAN_ONLY
// per-game start / end / placement plus 8 milestones (lane 0 stores s_memrealtime to g_span block
// 3 + mileOf(phase id)); no per-phase accumulation.  Each stamp costs an lgkmcnt drain and a store.
constexpr int NMILE = 8;
constexpr int mileOf(int ph) {
#ifdef MRTS_MILES_STEP  // multi-step analysis (tools/single_step_anatomy.py MILES=step): 0 = iteration start (after the
                        // view snapshot hand-off), 1 = the rows unpacked + issue index (selfPlayFast) instead of the load
    return ph == 0 ? 0 : ph == 22 ? 1 : ph == 1 ? 2 : ph == 3 ? 3 : ph == 4 ? 4 : ph == 5 ? 5 : ph == 6 ? 6 : ph == 9 ? 7 : -1;
#else
    return ph == 20 ? 0 : ph == 21 ? 1 : ph == 1 ? 2 : ph == 3 ? 3 : ph == 4 ? 4 : ph == 5 ? 5 : ph == 6 ? 6 : ph == 9 ? 7 : -1;
#endif
}
#ifdef MRTS_NO_MILESTONES  // start / end / placement only (tools/launch_gap.py)
#define PHASE_IN(acc, tt, i) \
    do {                     \
    } while (0)
#else
#define PHASE_IN(acc, tt, i)                                                                      \
    do {                                                                                          \
        if (mileOf(i) >= 0 && threadIdx.x == 0 && (int)blockIdx.x < PH_GAMES)                      \
            g_span[(3 + mileOf(i)) * PH_GAMES + blockIdx.x] = __builtin_amdgcn_s_memrealtime(); \
    } while (0)
#endif
#else
#define PHASE_IN(acc, tt, i)                          \
    do {                                              \
        const uint64_t t_ = __builtin_amdgcn_s_memtime(); \
        (acc)[i] += t_ - (tt);                        \
        (tt) = t_;                                    \
    } while (0)
#endif
#define PHASE(i) PHASE_IN(G.phAcc, G.tph_, i)  // in the kernel body
#define MPHASE(i) PHASE_IN(phAcc, tph_, i)     // inside Game methods
#else
#define PHASE(i) \
    do {         \
    } while (0)
#define MPHASE(i) \
    do {          \
    } while (0)
#endif
// Diagnostic build only (-DMRTS_ABLATE, `make ablate`; tools/ablate_price.py, tools/ablate_sq.py): a set bit of
// g_ablate runs its phase twice (idempotently, inputs laundered so the copies cannot be merged) — the marginal cost of
// a phase in the real, contended kernel — or leaves something out, or counts.  Never loaded by the package.  The bits,
// their kinds and names are the rows of mrts_ablate.h; a site in the step is one line of one of the three macros below,
// and a second copy longer than its line is a member of Game's last section (abl...).
#ifdef MRTS_ABLATE
#include "mrts_ablate.h"
__device__ uint64_t g_ablate;
__device__ unsigned long long g_dbg[4];  // diagnostics: [0] PO render items, [1] PO renders, [2] delta renders
template <class T>
DEV T launder(T v) {
    asm volatile("" : "+v"(v));
    return v;
}
template <class T>
DEV void keepv(T v) {
    asm volatile("" ::"v"(v));
}
#define X(n, bit, kind, name, steadyName) AB_##n = bit,
enum { MRTS_AB_PHASES(X) };
#undef X
#endif
// A site tests its bit through ab(b): Game's member, and in k_env a local of the same name.  Without MRTS_ABLATE
// AB_ON expands to nothing and the two prefixes to the bare statement that follows them.
#ifdef MRTS_ABLATE
#define AB_ON(b, ...) if (ab(b)) { __VA_ARGS__; } else (void)0  // the statement(s) if bit b: a phase once more; snapshot*()'s return
#define AB_SKIP(b) if (!ab(b))                                  // prefix: not the next statement if bit b
#define AB_TWICE(b) for (int rep_ = 0; rep_ < (ab(b) ? 2 : 1); rep_++)  // prefix: the next statement twice if bit b
#else
#define AB_ON(b, ...) (void)0
#define AB_SKIP(b)
#define AB_TWICE(b)
#endif
enum { GT_SELFPLAY = 0, GT_AGENT_VS_BOT = 1, GT_BOT_VS_BOT = 2, GT_PLAYOUT = 3 };  // game_kind & 15
// per-player counters of this step's issued pairs, as the TraceEntry holds them (after issueSafe's
// legality rewrite, before issue()'s conflict cancellations): HARVEST, RETURN, ATTACK, and PRODUCE
// of a Worker / a Base or Barracks / a Light, Heavy or Ranged
enum { RC_HARVEST = 0, RC_RETURN = 1, RC_ATTACK = 2, RC_PROD_WORKER = 3, RC_PROD_BUILDING = 4, RC_PROD_COMBAT = 5, RC_N = 6 };
DEV int prodCategory(uint32_t typeFlags) {  // the reward functions' name tests (DevUtt.flags N_*)
    return (typeFlags & N_WORKER) ? RC_PROD_WORKER : (typeFlags & N_BUILDING) ? RC_PROD_BUILDING
                                                   : (typeFlags & N_COMBAT) ? RC_PROD_COMBAT : -1;
}
enum { GK_PASSIVE = 0, GK_RANDOM_BIASED = 1, GK_LIGHT_RUSH = 2 };  // AI kinds (bits 4-7 ai1, 8-11 ai2)
enum : uint32_t {
    E_CAPACITY = 1u << 0, E_ADDUNIT = 1u << 1, E_PRODUCE_TYPE = 1u << 2, E_OLDER = 1u << 3,
    E_NEG_RES = 1u << 4, E_COLLISION = 1u << 5, E_RECORD = 1u << 6,
    E_INDEX = 1u << 7  // audit build only: the steady instance's carried issue index differs from a rebuilt one
};
// MODE_TRACE per-game result word (KDyn.trace_out)
enum : uint32_t { TR_ISSUED = 1u, TR_GAMEOVER = 2u, TR_NO_UNIT = 4u };

// branch-probability hints: cold paths (more than 64 units, auto-reset, conflict resolution, the
// general mask writer, reward bookkeeping the benchmark does not request) are laid out away from the
// hot straight-line code, which then packs into fewer instruction-cache lines
#define MRTS_LIKELY(x) __builtin_expect(!!(x), 1)
#define MRTS_UNLIKELY(x) __builtin_expect(!!(x), 0)
// The build switches that remain: the diagnostic builds above and MRTS_LANE_AUDIT (mrts_device.h), and the two that a
// committed test or tool builds at the other value.  An experiment's switch lives for the pull request that
// measures it (`make x1 XFLAGS1=-D...`); the code then keeps the measured choice.
#ifndef MRTS_ISSUE_BOTH  // selfPlayFast issues both players' rows in one pass when no row of either interacts (round 7);
#define MRTS_ISSUE_BOTH 1  // 0: tests/test_gpu_issue_both.py's comparison build
#endif
// 1: partially observable multi-step launches without the render helper wave (tools/po_helper_repro.py).  Round 4
// had made it the default after its full-size soak found 2 of 2048 c5 games with one stale observation value
// for a unit that died in the observed step; round 5 found the cause (the renders read the dead unit's
// fields by readlane inside their divergent chunk loop, from a lane that was off there — poChunk)
// and the helper is back on.
#ifndef MRTS_NO_PO_HELPER
#define MRTS_NO_PO_HELPER 0
#endif
// PO self-play: the views' base reservations in a bitmap of their own (selfPlayFast's `vres`; round 6: measured
// -0.5 % on c5, off).  Rejected, and still a switch: with its dead arm folded away the default library's device code
// stays byte-identical but the `timing` and `ablate` builds' does not (the early inliner sees other code), and the
// fold that retired the other switches rested on that identity.
#ifndef MRTS_PO_VRES
#define MRTS_PO_VRES 0
#endif
// The kernel's KDyn argument as a pointer into the constant (kernarg) address space.  The multi-step
// loop makes it opaque once per iteration (freshLane), so the compiler re-reads a field with a scalar
// load (SMEM) where the step uses it, instead of loading every field at kernel entry and keeping it
// live across the loop: that spilled ~240 SGPRs into VGPR lanes, and every reload was a v_readlane —
// a VALU instruction in a VALU-issue-bound kernel.
typedef const __attribute__((address_space(4))) KDyn* KDynPtr;
// k_env's KDyn argument: its third kernel argument, after the two pointers, at byte 16 of the kernarg
// segment.  The offset is laundered (not the address: an address escaping into asm makes the compiler
// copy the whole argument to scratch memory first).
static_assert(alignof(KDyn) <= 8, "k_env(int32_t*, const KStatic*, KDyn): KDyn at kernarg byte 16");
DEV KDynPtr kdynArg(bool launder) {
    int z = 0;
    if (launder) asm volatile("" : "+s"(z));
    return (KDynPtr)((const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr() + 16 + z);
}

// KDyn option tests that the steady instance (`steady`: Game's and k_env's template parameter) knows the answer to:
// D_HAS a buffer the steady state always has, D_OFF one it never has, D_ON a switch that is on, D_ZERO a value
// that is 0.  Every other instance reads the field.
#define D_HAS(f) (steady || D.f != nullptr)
#define D_OFF(f) (steady ? nullptr : D.f)
#define D_ON(f) (steady || D.f != 0)
#define D_ZERO(f) (steady ? 0 : D.f)
// steady: the game of k_env's STEADY instance (launchEnv's steadyLaunch picks it) — the launch is the fused self-play
// rollout's steady state, so the option tests such a launch never changes are constants
template <bool steady>
struct Game {
#define D (*Dp)
    const KStatic& P;
    KDynPtr Dp;  // the kernel argument itself (kernarg memory): fields load on demand
    const DevUtt& U;
    int g, H, W, HW, CAP;
    int K, NT, R;  // mask slots per cell, unit types, attack window (2 * max range + 1): table values or constants
    bool po;
    bool iter;        // a multi-step kernel (KDyn.n_iter iterations per launch)
    int32_t* stBase;  // the state blocks (a leading kernel argument: preloaded into SGPRs)
    int stWords;      // words per state block (a constant in a specialised kernel)
    uint32_t* uc;    // unit core: x | y<<8 | type<<16 | (player+1)<<20 | dead<<31
    uint32_t* ua;    // assignment: type | utype<<4 | tx<<8 | ty<<16 | PRESENT/READY/PA/DEC/BAD
    int32_t* at;     // assignment issue time (UnitActionAssignment.time)
    int32_t* as;     // assignment insertion sequence number (LinkedHashMap order)
    uint32_t* bits;  // running ResourceUsage positions, indices [-W, HW+W)
    uint32_t* scell; // PO: last snapshot unit per cell (slot+1, 0 = none)
    uint32_t* vis;   // PO: 2 x H rows x ceil(W/32) words of sight-disk bitmaps (after scell)
    // PO delta rendering (poDeltaShape maps only, after vis): the previous render's sight rows [view][2][H]
    // and dead-unit chunks [view][NCW], this view's dirty chunk bits [NCW] and chunk list [HW / 4]
    uint32_t* poVis;
    uint32_t* poPend;
    uint32_t* poDirty;
    uint32_t* vis2;  // writeObsPOFast2: view 1's sight rows [2][H]
    uint16_t* poList;
    int32_t* rseq;   // ready-list scratch (64)
    uint32_t* mprev; // previous mask row sets, [2][maskWords(HW)] (delta mask writes)
    int32_t* rwc;    // reward counters [player][RC_*] of the pairs issued this step
    int32_t* hdr;    // [32]: header words 0..15 (H_*) + HX_* extras
    int16_t* hp;
    int16_t* res;
    int16_t* par;    // UnitAction.parameter (direction / NONE duration)
    uint16_t* cell;  // cell -> slot, EMPTY or WALL
    uint16_t* rslot; // ready-list scratch (64)
    uint8_t* snap;   // PO snapshot bits
    // wave-uniform scalars (only ever modified in uniform control flow)
    int time, nu, pres0, pres1, seq, deaths;
    // Cold per-game scalars live in LDS (`hdr`), not in SGPRs: the header words H_* (steps, error
    // flags, cancel counter, kind, the three java.util.Random states) plus the HX_* extras below.
    // issue index (valid while ixValid): `bits` = target cells (+W) of present MOVE/PRODUCE
    // assignments, whether any exists, per player the largest present PRODUCE cost (-1 = none) and
    // the sum of present PRODUCE costs
#ifdef MRTS_PHASE_TIMING
    uint64_t tph_;
#ifndef MRTS_SPAN_ONLY
    uint64_t phAcc[NPH];  // per-phase cycles (registers: constant indices), flushed at kernel end
#endif
#endif
#ifdef MRTS_ABLATE
    // g_ablate's low word, read once by k_env and held through the step as before.  A row past bit 31 reads the high
    // word where it tests it (b is a constant at every site), so the wider word costs the step no register.
    uint32_t G_AB = 0;
    DEV bool ab(int b) const { return ((b < 32 ? G_AB : (uint32_t)(g_ablate >> 32)) >> (b & 31)) & 1u; }
#endif
    // lane id for the step code: threadIdx.x passed through an opaque (volatile asm) copy at the start
    // of every iteration of a multi-step launch, so that lane-derived values are recomputed per
    // iteration instead of being hoisted out of the loop and held in VGPRs across it (the loop alone
    // took k_env from 67 to 166 VGPRs: 3 waves per SIMD instead of the 4 the benchmark needs)
    // Only the multi-step kernels (iter, a compile-time constant after inlining) pay for it.
    int lidv;
    DEV int lid() const {
        if (!iter) return (int)threadIdx.x;
        __builtin_assume(lidv >= 0 && lidv < 64);
        return lidv;
    }
    DEV void freshLane() {
        if (iter) asm volatile("" : "=v"(lidv) : "0"((int)threadIdx.x));
        // multi-step kernels: the kernel argument's address made opaque again each step, so the fields
        // and addresses derived from it are re-read (SMEM) in the phase that uses them rather than held
        // across the step in spilled SGPRs (each reload a v_readlane)
        if (iter) Dp = kdynArg(true);
    }
    // the helper wave of a HELP launch (threads 64..127) runs Game methods as lanes 0..63
    DEV void helperLane() { asm volatile("" : "=v"(lidv) : "0"((int)threadIdx.x - 64)); }
    bool ixValid;
    bool anyMP;
    // steady instance: the index is carried from step to step of a launch (carryIndex); a present PRODUCE left
    // since the sums were last right (cycleLanes, kill), so they are walked again at the next step's start
    bool prodDirty = false;
    // steady instance: the own idle units the last writeMasksSteady of this launch found (-1 = none ran): the next
    // step's issue priority counts them, and nothing between the two changes a unit or an assignment
    int idleOwn = -1;
    // the PRODUCE costs of the issue index, the batch and the candidates summed by a walk over their
    // lanes instead of whole-wave reductions (the masked-policy 16x16 instances: few PRODUCE lanes;
    // c2's uniform rows make many, where the reductions are cheaper; round 5)
    bool walk;
    uint32_t lcu, lua;     // load(): lane l's unit core / assignment words (units 0..63) as loaded
    uint32_t lfwd;         // load(): lane l's forwarded action word (KDyn.fwd_read)
    bool fwdOn;            // this game's forwarded action words are current (H_FWD == fwd_stamp - 1)
    bool fwdWritten;       // this launch wrote the forwarded action words (store() stamps H_FWD)
    uint32_t lkey, lsnap;  // PO delta: lane l's hp | resources << 16 as loaded, its previous render's snapshot byte
    bool poLds;            // the last PO render (writeObsPOFast2) left its whole record in LDS as well
    // multi-step launch: this is the launch's last iteration (the state block's internal copies — the
    // mask row sets, the forwarded words — are stored then only); the first (the terrain plane,
    // static, is written by the first observation write of the launch only).  One step: both.
    bool lastIt, firstIt;
    uint64_t killedLanes;  // cycle(): ready-list lanes whose unit was killed earlier in the cycle
    int curP;              // player whose pa is being issued
    // CloserToEnemyBase/Unit: each player's first Base before the step (x | y << 8, -1 = none) and
    // the smallest squared distance from the OTHER player's mobile units to it, before the step
    int readySlot;         // per lane: the unit slot of ready item lid() (-1 outside cycle)
    uint32_t polStep;      // the fused policy's Philox step (D.pol_step, + 1 per iteration of a multi-step launch)
    uint32_t uniStep;      // the fused uniform policy's step (D.uni_step, likewise)
    // helper-wave launch (k_env HELP): this iteration's uniform rows, drawn by the helper wave,
    // packed (packFwd) per [player slot][cell]; null = draw them here (fetchRow)
    const uint32_t* helpRows = nullptr;
    // helper-wave launch, partially observable (k_env HELP && FPO): where writeMasksLanes leaves this
    // step's mask records, policy rows and vacated cells for the helper to store (null = store them here)
    uint32_t* recOut = nullptr;
    int maxProd0, maxProd1, sumProd0, sumProd1;

    // h, w, hw, cap: the map dimensions — compile-time constants in a specialised kernel (every LDS
    // array offset then folds to an immediate), else the kernel arguments
    DEV Game(const KStatic& p, const KDyn& d /* k_env's argument D; other fields read through kdynArg */, int32_t* stb, int stw, uint8_t* smem, int h, int w, int hw, int cap, bool partial,
             int k, int nt, int r, bool iterating = false, int game = -1, bool walk = false)
        : P(p), Dp(kdynArg(false)), U(*(const DevUtt*)smem), g(game >= 0 ? game : (int)blockIdx.x), H(h), W(w), HW(hw), CAP(cap), K(k), NT(nt), R(r),
          po(partial), iter(iterating), stBase(stb), stWords(stw), walk(walk) {
        uint8_t* q = smem + UTT_LDS;  // the unit-type table copy comes first (see copyUtt)
        uc = (uint32_t*)q; q += 4 * CAP;
        ua = (uint32_t*)q; q += 4 * CAP;
        at = (int32_t*)q; q += 4 * CAP;
        as = (int32_t*)q; q += 4 * CAP;
        bits = (uint32_t*)q; q += 4 * ((HW + 2 * W + 31) / 32);
        rseq = (int32_t*)q; q += 4 * 64;
        mprev = (uint32_t*)q; q += 8 * maskWords(HW);
        rwc = (int32_t*)q; q += 4 * 16;
        hdr = (int32_t*)q; q += 4 * 32;
        hp = (int16_t*)q; q += 2 * CAP;
        res = (int16_t*)q; q += 2 * CAP;
        par = (int16_t*)q; q += 2 * CAP;
        cell = (uint16_t*)q; q += 2 * HW;
        rslot = (uint16_t*)q; q += 2 * 64;
        snap = (uint8_t*)q; q += (CAP + 3) & ~3;
        scell = (uint32_t*)q;  // PO only, last: the offsets above do not depend on it
        vis = scell + HW;
        poVis = vis + 2 * H * ((W + 31) / 32);
        poPend = poVis + 4 * H;
        poDirty = poPend + 2 * poChunkWords(HW);  // [view][dirty, next pending bits] (view 1: writeObsPOFast2)
        vis2 = poDirty + 4 * poChunkWords(HW);
        poList = (uint16_t*)(vis2 + 2 * H);  // up to 2 x HW / 4 entries
        ixValid = false;
        fwdOn = false;
        fwdWritten = false;
        lfwd = 0;
        poLds = false;
        lastIt = true;
        firstIt = true;
        polStep = d.pol_step;
        uniStep = d.uni_step;
        freshLane();
    }
    // HX_*: snapshot sequence limits (PO), CloserToEnemy* base positions / old minimum distances
    enum { HX_SNAP = 16, HX_BASE = 18, HX_OLDSQ = 20, HX_POVALID = 22 };
    DEV int hget(int i) const { return uni(hdr[i]); }
    DEV void hset(int i, int v) const {
        if (lid() == 0) hdr[i] = v;
    }
    DEV void addErr(uint32_t bits) const {
        if (lid() == 0) hdr[H_ERR] |= (int32_t)bits;
    }
    DEV uint32_t errFlags() const { return (uint32_t)hget(H_ERR); }
    DEV JRand rngLoad(int i) const { return JRand{rng_of(hget(i), hget(i + 1))}; }
    DEV void rngStore(int i, const JRand& r) const {
        hset(i, (int)(uint32_t)r.s);
        hset(i + 1, (int)(uint32_t)(r.s >> 32));
    }
    DEV int pres(int p) const { return p == 0 ? pres0 : pres1; }
    DEV void addPres(int p, int v) {
        if (p == 0) pres0 += v;
        else pres1 += v;
    }
    DEV bool inb(int x, int y) const { return x >= 0 && x < W && y >= 0 && y < H; }
    DEV const int32_t* tmpl() const { return P.tmpl + P.tmpl_off[g]; }
    DEV int32_t* st() const { return stBase + (size_t)g * stWords; }

    // UnitAction.ETA (rts/UnitAction.java:307-329)
    DEV int eta(int t, int prm, int ut, int unitType) const {
        switch (t) {
            case T_NONE: return prm;
            case T_MOVE: return U.moveT[unitType];
            case T_ATTACK: return U.attackT[unitType];
            case T_HARVEST: return U.harvestT[unitType];
            case T_RETURN: return U.moveT[unitType];  // RETURN lasts moveTime (:321-322)
            case T_PRODUCE: return U.produceT[ut];
        }
        return 0;
    }
    // eta without the per-type branches (lane-varying t: the switch ran each case under its own exec mask):
    // produceT, moveT, attackT, harvestT are consecutive MAX_TYPES arrays of DevUtt, so the duration is one
    // LDS read at [array(t)][t == PRODUCE ? ut : unitType]; NONE keeps its parameter, unknown types 0
    DEV int etaFlat(int t, int prm, int ut, int unitType) const {
        static_assert(offsetof(DevUtt, moveT) == offsetof(DevUtt, produceT) + 4 * MAX_TYPES &&
                          offsetof(DevUtt, attackT) == offsetof(DevUtt, produceT) + 8 * MAX_TYPES &&
                          offsetof(DevUtt, harvestT) == offsetof(DevUtt, produceT) + 12 * MAX_TYPES,
                      "DevUtt duration arrays");
        // array per type (4 bits each): MOVE moveT (1), HARVEST harvestT (3), RETURN moveT (1), PRODUCE produceT (0),
        // ATTACK attackT (2)
        const int arr = (int)((0x201310u >> (4 * (t & 7))) & 15u);
        const int v = U.produceT[arr * MAX_TYPES + (t == T_PRODUCE ? ut : unitType)];
        return t == T_NONE ? prm : (t <= T_ATTACK ? v : 0);
    }
    DEV int etaSlot(int s) const {
        const uint32_t a = ua[s];
        return eta(ua_type(a), par[s], ua_ut(a), utyp(uc[s]));
    }

    // ------------------------------------------------------------------ state load / store
    DEV void setTerrainWord(int w, uint32_t v) {  // 4 terrain bytes -> cells 4w..4w+3
#pragma unroll
        for (int b = 0; b < 4; b++)
            if (4 * w + b < HW) cell[4 * w + b] = ((v >> (8 * b)) & 0xFFu) ? WALL : EMPTY;
    }
    DEV void initCells() {  // terrain walls from the map template
        const int32_t* t = tmpl() + T_TERR;
        for (int w = lid(); w < (HW + 3) / 4; w += 64) setTerrainWord(w, (uint32_t)t[w]);
        wsync();
    }
    DEV void copyUtt() {  // the LDS copy of the unit-type table, when load() does not fetch it
        const int32_t* ug = (const int32_t*)&P.utt;
        int32_t* ul = (int32_t*)&U;
        for (int i = lid(); i < UTT_WORDS; i += 64) ul[i] = ug[i];
        wsync();
    }
    DEV void storeTerrain() {  // the template's terrain words into the state block (at reset)
        const int32_t* t = tmpl() + T_TERR;
        int32_t* d = st() + stateTerrOff(CAP, HW);
        for (int w = lid(); w < (HW + 3) / 4; w += 64) d[w] = t[w];
    }
    DEV uint32_t* prevG() const { return (uint32_t*)(st() + H_WORDS + N_ARRAYS * CAP); }
    DEV void loadPrev() {  // previous mask row sets (delta mask writes), when not fetched by load()
        const uint32_t* pg = prevG();
        for (int i = lid(); i < 2 * maskWords(HW); i += 64) mprev[i] = pg[i];
        wsync();
    }
    DEV void placeUnits() {
        for (int i = lid(); i < nu; i += 64) {
            const uint32_t c = uc[i];
            if (!(c & UC_DEAD)) cell[uy(c) * W + ux(c)] = (uint16_t)i;
        }
        wsync();
    }
    DEV void loadHeader(const int32_t* s) { loadHeader(lid() < H_WORDS ? s[lid()] : 0); }
    DEV void loadHeader(int hv) {  // hv = header word lid() (lanes < H_WORDS)
        time = rl(hv, H_TIME);
        nu = rl(hv, H_NU);
        pres0 = rl(hv, H_RES0);
        pres1 = rl(hv, H_RES1);
        seq = rl(hv, H_SEQ);
        deaths = 0;
        const int l = lid();
        if (l < H_WORDS) hdr[l] = hv;
        else if (l < 32) hdr[l] = (l >= HX_BASE && l < HX_BASE + 2) ? -1 : (l >= HX_OLDSQ && l < HX_OLDSQ + 2) ? INF : 0;
    }
    // One global round trip: header, unit rows 0..63 (speculative — CAP >= 64), the terrain and the
    // previous mask row sets are all in flight before the first wait.
    DEV void load(bool wantPrev) {
        const int32_t* s = st();
        const int32_t* arr = s + H_WORDS;
        const int32_t* terr = s + stateTerrOff(CAP, HW);
        const int l = lid();
        const int TW = (HW + 3) / 4, PW = 2 * maskWords(HW);
        const int hv = l < H_WORDS ? s[l] : 0;
        const int32_t* ug = (const int32_t*)&P.utt;
        const int32_t u0 = ug[l], u1 = l + 64 < UTT_WORDS ? ug[l + 64] : 0, u2 = l + 128 < UTT_WORDS ? ug[l + 128] : 0;
        int32_t r[N_ARRAYS];
#pragma unroll
        for (int a = 0; a < N_ARRAYS; a++) r[a] = arr[a * CAP + l];
        const uint32_t tw = l < TW ? (uint32_t)terr[l] : 0u;
        const uint32_t pv = (wantPrev && l < PW) ? (uint32_t)arr[N_ARRAYS * CAP + l] : 0u;
        // forwarded action words (speculative: used only if H_FWD, in this same round, matches)
        const uint32_t fw = D_ON(fwd_read) ? (uint32_t)s[stateFwdOff(CAP, HW) + l] : 0u;
        // PO delta: the previous render's record, in the same memory round
        const bool poRec = po && D.obs_delta && D.po_prev && poDeltaShape(H, W);
        const int32_t* pr = poRec ? D.po_prev + (size_t)g * D.po_words : nullptr;
        const int NCW = poChunkWords(HW), SW = poSnapWords(CAP);
        int32_t prv0 = 0, prsb = 0, prvv = 0, prv2 = 0, prpd = 0;
        if (poRec) {
            prv0 = pr[0];
            prsb = pr[1 + (l >> 2)];
            prvv = l < 4 * H ? pr[1 + SW + l] : 0;
            prv2 = l + 64 < 4 * H ? pr[1 + SW + l + 64] : 0;
            prpd = l < 2 * NCW ? pr[1 + SW + 4 * H + l] : 0;
        }
        loadHeader(hv);
        MPHASE(20);
        lcu = (uint32_t)r[A_UC];
        lua = (uint32_t)r[A_UA];
        lfwd = fw;
        fwdOn = D_ON(fwd_read) && (uint32_t)rl(hv, H_FWD) == D.fwd_stamp - 1u;
        if (poRec) {
            lkey = (uint32_t)(uint16_t)r[A_HP] | ((uint32_t)(uint16_t)r[A_RES] << 16);
            lsnap = ((uint32_t)prsb >> (8 * (l & 3))) & 0xFFu;
            if (l < 4 * H) poVis[l] = (uint32_t)prvv;
            if (l + 64 < 4 * H) poVis[l + 64] = (uint32_t)prv2;
            if (l < 2 * NCW) poPend[l] = (uint32_t)prpd;
            if (l == 0) hdr[HX_POVALID] = prv0;
        }
        {
            int32_t* ul = (int32_t*)&U;
            ul[l] = u0;
            if (l + 64 < UTT_WORDS) ul[l + 64] = u1;
            if (l + 128 < UTT_WORDS) ul[l + 128] = u2;
        }
        if (l < nu) {
            uc[l] = (uint32_t)r[A_UC];
            hp[l] = (int16_t)r[A_HP];
            res[l] = (int16_t)r[A_RES];
            ua[l] = (uint32_t)r[A_UA];
            par[l] = (int16_t)r[A_PAR];
            at[l] = r[A_AT];
            as[l] = r[A_AS];
        }
        for (int i = l + 64; i < nu; i += 64) {
            uc[i] = (uint32_t)arr[A_UC * CAP + i];
            hp[i] = (int16_t)arr[A_HP * CAP + i];
            res[i] = (int16_t)arr[A_RES * CAP + i];
            ua[i] = (uint32_t)arr[A_UA * CAP + i];
            par[i] = (int16_t)arr[A_PAR * CAP + i];
            at[i] = arr[A_AT * CAP + i];
            as[i] = arr[A_AS * CAP + i];
        }
        if (l < TW) setTerrainWord(l, tw);
        for (int w = l + 64; w < TW; w += 64) setTerrainWord(w, (uint32_t)terr[w]);
        if (wantPrev) {
            if (l < PW) mprev[l] = pv;
            for (int i = l + 64; i < PW; i += 64) mprev[i] = prevG()[i];
        }
        wsync();
        MPHASE(21);
        placeUnits();
    }
    DEV void store() {
        int32_t* s = st();
        const int l = lid();
        int hv = l < H_WORDS ? hdr[l] : 0;
        switch (l) {
            case H_TIME: hv = time; break;
            case H_NU: hv = nu; break;
            case H_RES0: hv = pres0; break;
            case H_RES1: hv = pres1; break;
            case H_SEQ: hv = seq; break;
            case H_FWD: hv = fwdWritten ? (int)D.fwd_stamp : 0; break;
        }
        if (l < H_WORDS) st1<WT_STATE>(s + l, hv);
        int32_t* arr = s + H_WORDS;
        for (int i = l; i < nu; i += 64) {
            st1<WT_STATE>(arr + A_UC * CAP + i, (int32_t)uc[i]);
            st1<WT_STATE>(arr + A_HP * CAP + i, hp[i]);
            st1<WT_STATE>(arr + A_RES * CAP + i, res[i]);
            st1<WT_STATE>(arr + A_UA * CAP + i, (int32_t)ua[i]);
            st1<WT_STATE>(arr + A_PAR * CAP + i, par[i]);
            st1<WT_STATE>(arr + A_AT * CAP + i, at[i]);
            st1<WT_STATE>(arr + A_AS * CAP + i, as[i]);
        }
    }
    // Between two iterations of a multi-step launch (KDyn.n_iter): the state stays in LDS, so the
    // registers load() would set are re-derived from it — lane l's unit words, the forwarded action
    // word the previous iteration sampled (lfwd, kept in its register), the per-step header extras.
    DEV void nextStep() {
        freshLane();
        const int l = lid();
        wsync();
        lcu = uc[l];  // l < 64 <= CAP; selfPlayFast ignores lanes >= nu
        lua = ua[l];
        fwdOn = fwdWritten;
        // without forwarded words (more than 64 units) the next decode reads the rows the previous
        // iteration's policy stored to the action tensor, and a PO render that kept no LDS copy of
        // its record makes the next one re-read it: this wave's own plain stores, read back on the
        // same CU — a workgroup-scope fence (the stores' vmcnt drain, which also waits for the
        // iteration's observation stores: only when needed — c5 paid ~6 us per step draining them
        // every step; an agent-scope __threadfence would also write back the XCD's L2: 4x slower)
        const bool poRec = po && D.obs_delta && D.po_prev && poDeltaShape(H, W);
        const bool poReload = poRec && !poLds;  // a render that kept no LDS copy: re-read the record
        if (poReload || (!fwdWritten && !D_OFF(uni_actions))) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        fwdWritten = false;
        poLds = false;
        if (!steady) hset(H_NU, nu);  // "the loaded unit count" of this iteration (PO delta render)
        if (poRec && !poReload) {  // the previous render's record from its LDS copies
            lkey = (uint32_t)(uint16_t)hp[l] | ((uint32_t)(uint16_t)res[l] << 16);
            lsnap = snap[l];  // after the compaction = the record's snapshot bytes; before clearSnap
        } else if (poReload) {  // the previous render's record, as load() takes it
            const int32_t* pr = D.po_prev + (size_t)g * D.po_words;
            const int NCW = poChunkWords(HW), SW = poSnapWords(CAP);
            const int32_t prv0 = pr[0], prsb = pr[1 + (l >> 2)];
            const int32_t prvv = l < 4 * H ? pr[1 + SW + l] : 0, prv2 = l + 64 < 4 * H ? pr[1 + SW + l + 64] : 0;
            const int32_t prpd = l < 2 * NCW ? pr[1 + SW + 4 * H + l] : 0;
            lkey = (uint32_t)(uint16_t)hp[l] | ((uint32_t)(uint16_t)res[l] << 16);
            lsnap = ((uint32_t)prsb >> (8 * (l & 3))) & 0xFFu;
            if (l < 4 * H) poVis[l] = (uint32_t)prvv;
            if (l + 64 < 4 * H) poVis[l + 64] = (uint32_t)prv2;
            if (l < 2 * NCW) poPend[l] = (uint32_t)prpd;
            if (l == 0) hdr[HX_POVALID] = prv0;
        }
        if (!steady) ixValid = false;  // (steady: carried, see carryIndex)
        deaths = 0;
        polStep++;
        uniStep++;
        // (HX_POVALID stays: it is the PO render record's "views rendered", set by poRecordSnaps)
        // (steady: full observability and WinLoss alone — nothing reads the HX_* extras)
        if (!steady && l >= H_WORDS && l < 32 && l != HX_POVALID)
            hdr[l] = (l >= HX_BASE && l < HX_BASE + 2) ? -1 : (l >= HX_OLDSQ && l < HX_OLDSQ + 2) ? INF : 0;
        wsync();
    }
    // new GameState(PhysicalGameState.load(map)) — JNIGridnetClient.reset (tests/JNIGridnetClient.java:239-241).
    // envSteps is NOT part of it: VecClient.reset (tests/JNIGridnetVecClient.java:179-211) never touches
    // envSteps[]; only the auto-reset path zeroes it (:229,264-265,285).
    DEV void resetFromTemplate() {
        const int32_t* t = tmpl();
        const int nu_t = t[T_NU];
        time = 0;
        seq = 0;
        deaths = 0;
        if (steady) ixValid = false;  // every assignment is gone: the next step builds the index
        pres0 = t[T_RES0];
        pres1 = t[T_RES1];
        nu = nu_t;
        const int32_t* tu = t + tmplUnits(HW);
        for (int i = lid(); i < nu_t; i += 64) {
            uc[i] = (uint32_t)tu[i];
            hp[i] = (int16_t)tu[nu_t + i];
            res[i] = (int16_t)tu[2 * nu_t + i];
            ua[i] = 0;
            par[i] = -1;
            at[i] = 0;
            as[i] = 0;
        }
        wsync();
        for (int c = lid(); c < HW; c += 64)
            if (cell[c] != WALL) cell[c] = EMPTY;
        wsync();
        placeUnits();
    }

    // ------------------------------------------------------------------ row fetch + decode
    // UnitAction.fromVectorAction (rts/UnitAction.java:675-709) for every idle unit of the external
    // player(s), lane-parallel, in ONE round of global loads: a pure function of (row, unit).  The
    // decoded action is parked in the unit's empty assignment fields with UA_DEC.
    // JNIGridnetClientSelfPlay.gameStep's two issueSafe passes (tests/JNIGridnetClientSelfPlay.java:
    // 159-189) for a game whose units fit one wave, under full observability: predecode, then per
    // player the acceptance chain (PlayerAction.fromVectorAction), issueSafe of the accepted rows in
    // cell order and fillWithNones(gs, p, 1) in list order — the same sequence as predecode + decode +
    // issuePlayer, with each lane's own unit fields (load()'s registers) instead of LDS re-reads.
    // Between steps no unit is dead; decoded rows are never parked in LDS (every idle unit's
    // assignment is written by its issue or its fill).
    // Partially observable games too (round 5; all units in one wave, snapBothOk): Java decodes each player's
    // rows against that player's view (JNIGridnetClientSelfPlay.java:159-189, PlayerAction.fromVectorAction
    // on the PartiallyObservableGameState), which holds every own unit (sight covers its own cell) with the
    // assignments it has when the view is made — so the decode, fillWithNones and issueSafe are the full
    // state's; only the pa's base reservations come from the view (the assignments of the units in it,
    // baseReservations(p)), and the views' snapshots are taken in order: both memberships + view 0's
    // assignments before player 0 issues (snapshotBoth, or the helper wave's bytes: snapTaken), view 1's
    // assignments after (snapshotActions(1)).  The generic predecode + decode path did the same, slower.
    DEV void selfPlayFast(const int32_t* rows0, const int32_t* rows1, int s0, bool snapTaken = false) {
        const int l = lid();
        const uint32_t cu = lcu;
        const int pl = l < nu ? uplay(cu) : -1;
        const bool idle = pl >= 0 && !(lua & UA_PRESENT);
        int32_t a[7] = {0, 0, 0, 0, 0, 0, 0};
        // fwdOn: the previous launch's fused policy sampled this unit's row (the values it wrote to the
        // action tensor at this cell) and forwarded it in the state block (decodeFwd below, no fetch)
        if (!fwdOn && idle) fetchRow(pl == 0 ? rows0 : rows1, s0 + pl, uy(cu) * W + ux(cu), a);
        const bool useIx = !po && (HW + 2 * W + 31) / 32 <= 64;  // PO: the view's reservations (baseReservations)
        if (steady && useIx && ixValid) carryIndex();  // (useIx: a constant of the steady instance's shape)
        else if (useIx) buildIndex();  // while the rows are in flight
        // PO (round 6): each view's base reservations go to a bitmap of their own in the top words of `scell` (free
        // during the issue: the general render's scratch map is done with; a helper wave's packs and cell map end at
        // word 896 of 32x32's 1,024), so the issue index in `bits` stays valid across both players' issues instead of
        // being rebuilt after each view's acceptance chain
        const int NBv = (HW + 2 * W + 31) / 32;
        uint32_t* const vres = (MRTS_PO_VRES && po && NBv <= 64 && HW - NBv >= (HW == 1024 ? 896 : 0)) ? scell + (HW - NBv) : nullptr;
        if (useIx) AB_ON(AB_INDEX, buildIndex());
        MPHASE(22);
        int t = 0, pr = -1, ut = 0, tx = 0, ty = 0;
        bool bad = false;
        // (in place: as a member of the copies' section it cost the 8x8 helper instance two more spilled VGPRs)
        AB_ON(AB_DECODE, if (idle) {
            int32_t b2[7];
            for (int k = 0; k < 7; k++) b2[k] = launder(a[k]);
            int t2 = 0, pr2 = -1, ut2 = 0, tx2 = 0, ty2 = 0;
            const bool bad2 = decodeFields(launder(cu), b2, t2, pr2, ut2, tx2, ty2);
            keepv(t2 + pr2 + ut2 + tx2 + ty2 + (int)bad2);
        });
        // steady, from the launch's second step on: writeMasksSteady left this row decoded in lfwd (sampledDec)
        const bool dec = steady && fwdOn && !firstIt;
        if (dec) {
            if (idle) {
                t = ua_type(lfwd);
                ut = ua_ut(lfwd);
                tx = ua_tx(lfwd);
                ty = ua_ty(lfwd);
                pr = (int)(lfwd >> 24) - 1;
            }
        } else if (idle) {
            bad = fwdOn ? decodeFwd(cu, lfwd, t, pr, ut, tx, ty) : decodeFields(cu, a, t, pr, ut, tx, ty);
        }
        AB_ON(AB_DECFWD, ablDecFwd(idle, dec, cu));
        if (ballot(bad)) addErr(E_PRODUCE_TYPE);
        const uint32_t adec = dec ? (idle ? lfwd & 0xFFFFFFu : 0u) : pack_ua(t, ut, tx, ty);
        const int c = uy(cu) * W + ux(cu);
        MPHASE(1);
        bool merged = false;
#if MRTS_ISSUE_BOTH
        // both players' rows in one pass when none interacts (issueBothTest); not with the reward counters
        // (issueBatch books them per player)
        if (useIx && MRTS_LIKELY(!(D_ZERO(reward_need) & RN_COUNTS))) {
            int s0, s1, mc0, mc1;
            const bool both = issueBothTest(idle && !bad, cu, adec, pr, s0, s1, mc0, mc1);
#ifdef MRTS_PHASE_TIMING
#ifndef MRTS_SPAN_ONLY
            phAcc[25] += 1000;  // merged issue: attempts, and hits (x1000 each)
            if (both) phAcc[26] += 1000;
#endif
#endif
            MPHASE(2);
            if (both) {
                AB_ON(AB_ISSUE, ablIssueBoth(idle && !bad, bad, cu, adec, pr));
                issueBothWrite(idle && !bad, bad, cu, adec, pr, s0, s1, mc0, mc1);
                MPHASE(3);
                merged = true;
            }
        }
#endif
        // (the merged pass skips the loop rather than returning: with the early return the c3 kernel's register
        // allocation spilled 19 VGPRs in the mask phase instead of 4)
        for (int p = merged ? 2 : 0; p < 2; p++) {
            if (po) {  // the views, in Java's order (see above)
                if (p == 0) {
                    if (!snapTaken) snapshotBoth();
                } else {
                    snapshotActions(1);
                }
            }
            int run0, run1;
            if (useIx) {
                if (!ixValid) buildIndex();
                run0 = sumProd0;
                run1 = sumProd1;
            } else {
                baseReservations(p, run0, run1, vres);
            }
            curP = p;
            const bool mine = idle && pl == p;
            const bool cand = mine && !bad;
            const uint64_t m = ballot(cand);
            bool isPA = false;
            if (m) {
                const int rank = cellRank(m, cand, c);
                AB_ON(AB_RANK, keepv(cellRank(m, cand, launder(c))));
                AB_ON(AB_ACCEPT, ablAccept(p, run0, run1, cand, rank, __popcll(m), t, pr, c, adec));
                MPHASE(23);
                int irank = 0;
                const uint64_t acc = acceptChain(p, run0, run1, cand, rank, __popcll(m), t, pr, c, adec, useIx || vres, irank, vres);
                MPHASE(2);
                isPA = (acc >> l) & 1ull;
                int tt = 0, prm = 0, ttx = 0, tty = 0, tut = 0;
                if (isPA) {
                    tt = t;
                    prm = pr;
                    ttx = tx;
                    tty = ty;
                    tut = ut;
                    AB_ON(AB_LEGAL, ablLegal(l, cu, t, pr, tx, ty, ut));
                    // A forwarded row was sampled by the fused policy from this unit's mask record, which
                    // the previous step wrote from this same state (no cycle in between): its type bit
                    // and parameter bits are members of getUnitActions' list (a PRODUCE's free
                    // directions x affordable types is a full product), and issuing the other player's
                    // pairs changes nothing the test reads (positions, hp, resources move only in
                    // cycle) — so issueSafe's legality test returns the row unchanged and is skipped.
                    // Any other row (the caller's tensor, the uniform policy) is tested.
                    if (!fwdOn) legality(l, cu, tt, prm, ttx, tty, tut);
                }
                wsync();
                MPHASE(24);
                if (acc) issueBatch(isPA, irank, __popcll(acc), l, tt, prm, ttx, tty, tut, false, &cu, nullptr, true);
            }
            // fillWithNones(gs, p, 1): p's idle units left without an action, list order
            const bool fill = mine && !isPA;
            const uint64_t mf = ballot(fill);
            if (fill) {
                ua[l] = pack_ua(T_NONE, 0, 0, 0) | UA_PRESENT;
                par[l] = 1;
                at[l] = time;
                as[l] = seq + lanes_below(mf);
            }
            seq += __popcll(mf);
            wsync();
            MPHASE(3);
        }
    }
    // The PRODUCE lanes' costs per player (sum, largest) added to s0 / s1 / mc0 / mc1: a walk over their
    // lanes, or whole-wave reductions (see `walk`)
    DEV void prodCosts(bool np, int cost, int pl, int& s0, int& s1, int& mc0, int& mc1) const {
        if (walk) {
            for (uint64_t mm = ballot(np); mm; mm &= mm - 1) {
                const int kv = uni(rl(cost | (pl << 16), __builtin_ctzll(mm)));
                const int k = kv & 0xFFFF;
                if ((kv >> 16) == 0) {
                    mc0 = max(mc0, k);
                    s0 += k;
                } else {
                    mc1 = max(mc1, k);
                    s1 += k;
                }
            }
        } else if (ballot(np)) {
            mc0 = max(mc0, -wave_min(np && pl == 0 ? -cost : 1));
            mc1 = max(mc1, -wave_min(np && pl == 1 ? -cost : 1));
            s0 += wave_sum(np && pl == 0 ? cost : 0);
            s1 += wave_sum(np && pl == 1 ? cost : 0);
        }
    }
    // selfPlayFast's two issueSafe passes as one (round 7), for the step in which no
    // candidate row of either player interacts with a reservation or with another row:
    //  (a) no MOVE / PRODUCE candidate of either player uses a position that is reserved already or that
    //      another candidate uses (the ResourceUsage positions, PlayerAction.java:400-415), and
    //  (b) per player, the present PRODUCE costs plus every candidate's cost fit the resources
    //      (ResourceUsage.java:31-50).
    // Then player 0's acceptance chain accepts every row (its parallel form's own condition), so does
    // player 1's against the reservations with player 0's rows added ((a) covers them, (b) keeps either
    // player's running sum from blocking the other), and every GameState.issue (GameState.java:252-326)
    // of either pa takes its no-conflict branch: each cost test there is a single or pairwise sum bounded
    // by (b)'s totals.  issueSafe's legality rewrite (:338-408) only turns rows into NONE, which removes
    // users of (a) and (b).  The state after both passes is then a function of the union of the rows:
    // the insertion order is [p0 accepted, by cell][p0 fills][p1 accepted, by cell][p1 fills].
    // The test writes nothing but the `rseq` scratch; false = not taken, nothing changed.
    DEV bool issueBothTest(bool cand, uint32_t cu, uint32_t adec, int pr, int& s0, int& s1, int& mc0, int& mc1) const {
        const int l = lid();
        const int NB = (HW + 2 * W + 31) / 32;
        const int t = ua_type(adec);
        const bool up = cand && (t == T_MOVE || t == T_PRODUCE), prod = cand && t == T_PRODUCE;
        const int tpos = (uy(cu) + dyo(pr) + 1) * W + ux(cu) + dxo(pr);  // ResourceUsage position, as acceptChain
        uint32_t* cp = (uint32_t*)rseq;  // free here (acceptChainReg's own copy lives there too)
        if (l < NB) cp[l] = bits[l];
        wsync();
        bool conf = false;
        if (up) conf = (atomicOr(&cp[tpos >> 5], 1u << (tpos & 31)) >> (tpos & 31)) & 1u;
        wsync();
        s0 = sumProd0;
        s1 = sumProd1;
        mc0 = maxProd0;
        mc1 = maxProd1;
        prodCosts(prod, prod ? U.cost[ua_ut(adec)] : 0, uplay(cu), s0, s1, mc0, mc1);
        return !ballot(conf) && s0 <= pres0 && s1 <= pres1;
    }
    // the writes of both pa's after issueBothTest passed: s0 / s1 / mc0 / mc1 are its PRODUCE sums
    DEV void issueBothWrite(bool cand, bool bad, uint32_t cu, uint32_t adec, int pr, int s0, int s1, int mc0, int mc1) {
        const int l = lid();
        const int pl = uplay(cu);
        const uint64_t mU = ballot(cand);
        const int n1 = __popcll(ballot(cand && pl == 1)), n0 = __popcll(mU) - n1;
        // rank among the union by (player, cell): player 0's rows are ranked by cell as cellRank does,
        // player 1's follow (their rank by cell + n0)
        const int key = (int)(((cu >> 20) & 3) << 16 | (cu & 0xFFFFu));  // player + 1, y, x
        int r = 0;
        for (uint64_t mm = mU; mm; mm &= mm - 1) r += rl(key, __builtin_ctzll(mm)) < key;
        // fillWithNones of each player: its idle units left without a row (bad produce type), list order
        const uint64_t mfU = ballot(bad);
        int f0 = 0;
        if (MRTS_UNLIKELY(mfU != 0)) {
            const uint64_t mf1 = ballot(bad && pl == 1), mf0 = mfU & ~mf1;
            f0 = __popcll(mf0);
            if (bad) {
                ua[l] = pack_ua(T_NONE, 0, 0, 0) | UA_PRESENT;
                par[l] = 1;
                at[l] = time;
                as[l] = seq + (pl == 0 ? n0 + lanes_below(mf0) : n0 + f0 + n1 + lanes_below(mf1));
            }
        }
        const bool prodRow = cand && ua_type(adec) == T_PRODUCE;
        if (!fwdOn) {  // as selfPlayFast: forwarded rows are legal, any other is tested
            int t = ua_type(adec), ut = ua_ut(adec), tx = ua_tx(adec), ty = ua_ty(adec);
            if (cand) legality(l, cu, t, pr, tx, ty, ut);
            adec = pack_ua(t, ut, tx, ty);
            wsync();
        }
        const int t = ua_type(adec);
        const bool mp = cand && (t == T_MOVE || t == T_PRODUCE), np = cand && t == T_PRODUCE;
        if (cand) {
            ua[l] = adec | UA_PRESENT;
            par[l] = (int16_t)pr;
            at[l] = time;
            as[l] = seq + r + (pl == 0 ? 0 : f0);
            // a legal MOVE / PRODUCE keeps its direction: the issue index takes the position the test used
            const int tpos = (uy(cu) + dyo(pr) + 1) * W + ux(cu) + dxo(pr);
            if (mp) atomicOr(&bits[tpos >> 5], 1u << (tpos & 31));
        }
        seq += __popcll(mU) + __popcll(mfU);
        if (ballot(mp)) anyMP = true;
        if (!fwdOn && ballot(prodRow && !np)) {  // a PRODUCE row became NONE: the sums of those that stayed
            s0 = sumProd0;
            s1 = sumProd1;
            mc0 = maxProd0;
            mc1 = maxProd1;
            prodCosts(np, np ? U.cost[ua_ut(adec)] : 0, pl, s0, s1, mc0, mc1);
        }
        sumProd0 = s0;
        sumProd1 = s1;
        maxProd0 = mc0;
        maxProd1 = mc1;
        curP = 1;
        wsync();
    }
    // Row of cell c of slot `slot` (rows = that slot's rows): the action tensor's, or, in a fused
    // uniform-policy step (KDyn.uni_actions), the Philox row the launch also writes there
    // (writeUniformRows) — drawn again in registers instead of read back.
    DEV void fetchRow(const int32_t* rows, int slot, int c, int32_t a[7]) const {
        if (helpRows) {  // the helper wave drew this step's rows (self-play: slot & 1 = player)
            unpackFwd(helpRows[(slot & 1) * HW + c], a);
            return;
        }
        if (D.uni_actions) {
            uniformRow(D.uni_seed, uniStep, D.uni_slot_base + (uint32_t)slot, c, NT, K - 23 - NT, a);
            return;
        }
        const int32_t* r = rows + (size_t)c * 7;
#pragma unroll
        for (int k = 0; k < 7; k++) a[k] = r[k];
    }
    // the fused uniform policy's output: every row of this game's slots, as k_policy_uniform writes them
    DEV void writeUniformRows(int slot0, int nslots) const {
        for (int i = 0; i < nslots; i++)
            for (int c = lid(); c < HW; c += 64) {
                int32_t a[7];
                uniformRow(D.uni_seed, uniStep, D.uni_slot_base + (uint32_t)(slot0 + i), c, NT, K - 23 - NT, a);
                int32_t* dst = D.uni_actions + ((size_t)(slot0 + i) * HW + c) * 7;
                st4u<false>(dst, a[0], a[1], a[2], a[3]);
                st3u<false>(dst + 4, a[4], a[5], a[6]);
            }
    }
    DEV void predecode(const int32_t* rows0, const int32_t* rows1, int only, int s0, int s1) {
        bool bad_any = false;
        const int l = lid();
        // units 0..63: rows requested first, the issue index (LDS only) is built while they are in
        // flight, then decoded
        int32_t a[7] = {0, 0, 0, 0, 0, 0, 0};
        bool act = false;
        if (l < nu) {
            const uint32_t cu = uc[l];
            const int pl = uplay(cu);
            act = !(pl < 0 || (ua[l] & UA_PRESENT) || (only >= 0 && pl != only));
            if (act) {
                // units 0..63 of a self-play game: the fused policy's forwarded word when current
                // (as selfPlayFast), else the action tensor
                if (fwdOn) unpackFwd(lfwd, a);
                else fetchRow(pl == 0 ? rows0 : rows1, pl == 0 ? s0 : s1, uy(cu) * W + ux(cu), a);
            }
        }
        if (!po && (HW + 2 * W + 31) / 32 <= 64) buildIndex();
        if (act) bad_any |= decodeRow(l, a);
        for (int o = l + 64; o < nu; o += 64) {
            const uint32_t cu = uc[o];
            const int pl = uplay(cu);
            if (pl < 0 || (ua[o] & UA_PRESENT) || (only >= 0 && pl != only)) continue;
            int32_t b[7];
            fetchRow(pl == 0 ? rows0 : rows1, pl == 0 ? s0 : s1, uy(cu) * W + ux(cu), b);
            bad_any |= decodeRow(o, b);
        }
        if (ballot(bad_any)) addErr(E_PRODUCE_TYPE);
        wsync();
    }
    // UnitAction.fromVectorAction of row a for unit o; returns "produce type out of range"
    DEV bool decodeRow(int o, const int32_t a[7]) {
        int t, pr, ut, tx, ty;
        const bool bad = decodeFields(uc[o], a, t, pr, ut, tx, ty);
        ua[o] = pack_ua(t, ut, tx, ty) | UA_DEC | (bad ? UA_BAD : 0u);
        par[o] = (int16_t)pr;
        return bad;
    }
    // UnitAction.fromVectorAction (rts/UnitAction.java:675-709) of row components a[0..6] for a unit
    // with core word cu
    // Branch-free (selects only): the lanes of one wave hold rows of every type, and a divergent switch
    // runs each present case's instructions for the whole wave.
    // decodeFields(cu, unpackFwd(w)) straight from a forwarded action word: the direction field picked by
    // the type with one bit-field extract instead of unpacking all seven values and selecting among them
    // decodeFwd of the row the fused policy's sampler just drew, from its picks (sampleBitsRaw: type t, parameter
    // pick pv, produce type ut) for the unit with core word cu: pack_ua(t, ut, tx, ty) | (parameter + 1) << 24.  The
    // picks are members of the unit's mask record, so the tests decodeFwd makes of a foreign row are decided: a
    // direction is 0..3, a produce type is in the table, an attack target is a unit's cell (on the map).
    DEV uint32_t sampledDec(uint32_t cu, int t, int pv, int ut) const {
        // the target cell of window index pv, x | y << 8 in one sum: the unit's x | y << 8, plus pv % R | pv / R << 8
        // (= pv + (256 - R) (pv / R)), minus the window's centre in both bytes (no byte borrows: the cell is on the map)
        const uint32_t q = R == 7 ? ((uint32_t)pv * 37u) >> 8 /* pv / 7 for pv < 56 */ : (uint32_t)pv / (uint32_t)R;
        const uint32_t ctr = (uint32_t)(R / 2);
        const uint32_t xy = (cu & 0xFFFFu) + (uint32_t)pv + q * (uint32_t)(256 - R) - (ctr | ctr << 8);
        const bool dirT = (uint32_t)(t - T_MOVE) <= (uint32_t)(T_PRODUCE - T_MOVE);
        return (uint32_t)t | (uint32_t)ut << 4 | (t == T_ATTACK ? xy << 8 : 0u) | (dirT ? (uint32_t)(pv + 1) << 24 : 0u);
    }
    DEV bool decodeFwd(uint32_t cu, uint32_t w, int& t, int& pr, int& ut, int& tx, int& ty) const {
        const int ctr = R / 2;
        const int x = ux(cu), y = uy(cu);
        const int a0 = (int)(w & 7u);
        t = a0 <= 5 ? a0 : ACT_INVALID;
        const bool dirT = t >= T_MOVE && t <= T_PRODUCE;
        const int d = (int)__builtin_amdgcn_ubfe(w, 3u * (uint32_t)(dirT ? t : T_PRODUCE), 3u) - 1;  // a[t] (a[4] otherwise)
        pr = dirT ? clampdir(d) : -1;
        const bool prod = t == T_PRODUCE;
        const int a5 = (int)((w >> 15) & 15u) - 1, a6 = (int)((w >> 19) & 127u) - 1;
        const bool badType = a5 < 0 || a5 >= NT;
        ut = (prod && !badType) ? a5 : 0;
        const int ax = x + (a6 % R - ctr), ay = y + (a6 / R - ctr);
        const bool att = t == T_ATTACK, on = inb(ax, ay);
        tx = att ? (on ? ax : 255) : 0;
        ty = att ? (on ? ay : 255) : 0;
        return prod && badType;
    }
    DEV bool decodeFields(uint32_t cu, const int32_t a[7], int& t, int& pr, int& ut, int& tx, int& ty) const {
        const int ctr = R / 2;
        const int x = ux(cu), y = uy(cu);
        t = (a[0] >= 0 && a[0] <= 5) ? a[0] : ACT_INVALID;
        // MOVE / HARVEST / RETURN / PRODUCE: the direction of that type's component
        const int d = t == T_MOVE ? a[1] : t == T_HARVEST ? a[2] : t == T_RETURN ? a[3] : a[4];
        pr = (t >= T_MOVE && t <= T_PRODUCE) ? clampdir(d) : -1;
        // PRODUCE: utt.getUnitType(int) throws for a type outside the table (:697)
        const bool prod = t == T_PRODUCE;
        const bool badType = a[5] < 0 || a[5] >= NT;
        ut = (prod && !badType) ? a[5] : 0;
        // ATTACK: the target cell of the window index, off-map -> never legal
        const int ax = x + (a[6] % R - ctr), ay = y + (a[6] / R - ctr);
        const bool att = t == T_ATTACK, on = inb(ax, ay);
        tx = att ? (on ? ax : 255) : 0;
        ty = att ? (on ? ay : 255) : 0;
        return prod && badType;
    }

    // ------------------------------------------------------------------ Java row layout
    // PlayerAction.fromVectorAction over Java rows [pos, 7 comps] in list order (rts/PlayerAction.java:
    // 384-417): a row counts iff an own unit with no assignment stands at (pos % W, pos / W); rows may
    // name a unit twice (both can be accepted).  Accepted pairs go, in order, to the game's scratch.
    // Returns the pair count.
    DEV int rowsDecode(int p, const int32_t* rows) {
        int run0, run1;
        baseReservations(p, run0, run1);
        const int l = lid();
        uint32_t* pairs = D.pairs + (size_t)g * D.n_rows * 2;
        int npairs = 0;
        bool badAny = false;
        for (int r0 = 0; r0 < D.n_rows; r0 += 64) {
            const int r = r0 + l;
            int32_t a[8] = {-1, 0, 0, 0, 0, 0, 0, 0};
            if (r < D.n_rows)
#pragma unroll
                for (int k = 0; k < 8; k++) a[k] = rows[(size_t)r * 8 + k];
            const int pos = a[0];
            bool cand = false;
            int s = 0, t = 0, pr = 0, ut = 0, tx = 0, ty = 0;
            uint32_t cu = 0;
            if (pos >= 0 && pos < HW) {
                s = cell[pos];
                if (s < CAP) {
                    cu = uc[s];
                    cand = uplay(cu) == p && !(ua[s] & UA_PRESENT);
                }
            }
            if (cand) {
                const bool bad = decodeFields(cu, a + 1, t, pr, ut, tx, ty);
                badAny |= bad;
                cand = !bad;  // Java throws here (UnitAction.java:697): reported as E_PRODUCE_TYPE
            }
            const uint64_t m = ballot(cand);
            if (m == 0) continue;
            const uint32_t av = pack_ua(t, ut, 0, 0);
            int irank = 0;
            const uint64_t acc = acceptChain(p, run0, run1, cand, cand ? lanes_below(m) : -1, __popcll(m), t, pr, pos, av, false, irank);
            if ((acc >> l) & 1ull) {
                const int idx = npairs + lanes_below(acc);
                pairs[(size_t)idx * 2] = (uint32_t)s | ((uint32_t)t << 16) | ((uint32_t)ut << 20);
                pairs[(size_t)idx * 2 + 1] = (uint32_t)(uint16_t)pr | ((uint32_t)tx << 16) | ((uint32_t)ty << 24);
            }
            npairs += __popcll(acc);
        }
        if (ballot(badAny)) addErr(E_PRODUCE_TYPE);
        __threadfence();  // the pairs are read back (by other lanes) in rowsIssue
        return npairs;
    }
    // issueSafe(pa) for the pairs of rowsDecode + fillWithNones(gs, p, fillDur) (PlayerAction.java:217-235)
    DEV void rowsIssue(int p, int npairs, int fillDur) {
        curP = p;
        const uint32_t* pairs = D.pairs + (size_t)g * D.n_rows * 2;
        for (int b0 = 0; b0 < npairs; b0 += 64) {
            const int k = b0 + lid();
            const bool act = k < npairs;
            int s = 0, t = 0, prm = 0, tx = 0, ty = 0, ut = 0;
            if (act) {
                const uint32_t w0 = pairs[(size_t)k * 2], w1 = pairs[(size_t)k * 2 + 1];
                s = (int)(w0 & 0xFFFFu);
                t = (int)((w0 >> 16) & 0xFu);
                ut = (int)((w0 >> 20) & 0xFu);
                prm = (int)(int16_t)(w1 & 0xFFFFu);
                tx = (int)((w1 >> 16) & 0xFFu);
                ty = (int)(w1 >> 24);
                legality(s, t, prm, tx, ty, ut);
            }
            wsync();
            issueBatch(act, lid(), min(64, npairs - b0), s, t, prm, tx, ty, ut, true);
        }
        issueFills(p, fillDur);
    }

    // ------------------------------------------------------------------ trace replay (MODE_TRACE)
    // issueSafe(pa) (rts/GameState.java:338-408) of player p's pairs of a trace entry, as
    // TestTracesIntegrity.testTrace builds them (test/microrts/TestTracesIntegrity.java:101-121): rows
    // [player, x, y, type, parameter, target x, target y, unit type], the player's rows in the given
    // order.  Each action's legality is judged on the trace's own Unit object, whose fields equal those
    // of the state's unit at (x, y) whenever the replay is in sync; that unit is then the one issued —
    // the first unit at (x, y) in list order (GameState.java:356-382; one unit per cell).  No fillWithNones.
    // Returns issue()'s value: a pair was put with a type other than NONE.
    DEV bool traceIssue(int p, const int32_t* rows, int n, uint32_t& flags) {
        curP = p;
        bool put = false;
        bool missing = false;
        for (int r0 = 0; r0 < n; r0 += 64) {
            const int r = r0 + lid();
            int32_t a[8] = {-1, 0, 0, 0, 0, 0, 0, 0};
            if (r < n)
#pragma unroll
                for (int k = 0; k < 8; k++) a[k] = rows[(size_t)r * 8 + k];
            bool act = a[0] == p;
            int s = 0;
            if (act) {
                s = inb(a[1], a[2]) ? (int)cell[a[2] * W + a[1]] : EMPTY;
                if (s >= CAP) {  // no unit there: Java prints "Inconsistent order" and issues the trace's unit
                    missing = true;
                    act = false;
                }
            }
            int t = a[3], prm = a[4], tx = 0, ty = 0, ut = 0;
            if (act) {
                if (t < T_NONE || t > T_ATTACK) t = ACT_INVALID;  // never in getUnitActions: NONE(0)
                const bool dir = t >= T_MOVE && t <= T_PRODUCE;
                if (dir && (prm < 0 || prm > 3)) prm = 4;  // not a direction: never legal
                if (t == T_PRODUCE) ut = a[7];              // the host checked 0 <= ut < ntypes
                if (t == T_ATTACK) {
                    const bool on = inb(a[5], a[6]);
                    tx = on ? a[5] : 255;
                    ty = on ? a[6] : 255;
                }
                legality(s, t, prm, tx, ty, ut);
            }
            const uint64_t m = ballot(act);
            wsync();
            if (m) issueBatch(act, act ? lanes_below(m) : 0, __popcll(m), s, t, prm, tx, ty, ut, true, nullptr, &put);
        }
        if (ballot(missing)) flags |= TR_NO_UNIT;
        return put;
    }

    // Base reservations of every current assignment the deciding view holds (PlayerAction.java:387-394,
    // merged as ResourceUsage.java:92-97); in a PO view only snapshot units' assignments count.
    // tgt: the bitmap to fill (null: `bits`, which then no longer holds the issue index)
    DEV void baseReservations(int p, int& r0, int& r1, uint32_t* tgt = nullptr) {
        const int NB = (HW + 2 * W + 31) / 32;
        uint32_t* const bits = tgt ? tgt : this->bits;
        if (!tgt) ixValid = false;  // `bits` now holds this view's set
        for (int i = lid(); i < NB; i += 64) bits[i] = 0;
        wsync();
        int s0 = 0, s1 = 0, w0 = 0, w1 = 0;
        for (int o0 = 0; o0 < nu; o0 += 64) {
            const int o = o0 + lid();
            int key = -1;  // walk: a PRODUCE's cost | player << 16
            if (o < nu) {
                const uint32_t a = ua[o];
                const int t = ua_type(a);
                if ((a & UA_PRESENT) && (!po || snap_in(snap[o], p)) && (t == T_MOVE || t == T_PRODUCE)) {
                    const uint32_t c = uc[o];
                    const int d = par[o];
                    const int pos = (uy(c) + dyo(d)) * W + ux(c) + dxo(d) + W;
                    atomicOr(&bits[pos >> 5], 1u << (pos & 31));
                    if (t == T_PRODUCE) {
                        key = U.cost[ua_ut(a)] | ((uplay(c) == 0 ? 0 : 1) << 16);
                        if (uplay(c) == 0) s0 += U.cost[ua_ut(a)];
                        else s1 += U.cost[ua_ut(a)];
                    }
                }
            }
            if (walk) {  // the few PRODUCE lanes: one lane read each (buildIndex's walk)
                for (uint64_t mm = ballot(key >= 0); mm; mm &= mm - 1) {
                    const int kv = uni(rl(key, __builtin_ctzll(mm)));
                    if ((kv >> 16) == 0) w0 += kv & 0xFFFF;
                    else w1 += kv & 0xFFFF;
                }
            }
        }
        if (walk) {
            r0 = w0;
            r1 = w1;
        } else {
            r0 = wave_sum(s0);
            r1 = wave_sum(s1);
        }
        wsync();
    }

    // PlayerAction.fromVectorAction (rts/PlayerAction.java:384-417): decoded rows in ascending cell
    // order; accepted iff ua.ru.consistentWith(running ru) (rts/ResourceUsage.java:31-50).  Only the
    // acceptance chain is serial; accepted units get UA_PA.
    // issueNow (self-play, all units in one wave): the accepted rows are issued straight from the
    // chain's registers — issueSafe(pa) of the same pairs in the same (cell) order as issuePlayer
    DEV void decode(int p, bool issueNow = false) {
        int run0, run1;
        // full observability: the base reservations are the issue index (every present MOVE/PRODUCE
        // target + per-player PRODUCE cost sums), kept current across issue batches
        const bool useIx = !po && (HW + 2 * W + 31) / 32 <= 64;
        if (useIx) {
            if (!ixValid) buildIndex();
            run0 = sumProd0;
            run1 = sumProd1;
        } else {
            baseReservations(p, run0, run1);
        }
        MPHASE(13);
        if (MRTS_LIKELY(nu <= 64)) {
            decodeUnits(p, run0, run1, useIx, issueNow);
            return;
        }
        ixValid = false;  // the chain below adds to `bits`
        for (int c0 = 0; c0 < HW; c0 += 64) {
            const int c = c0 + lid();
            const int s = c < HW ? cell[c] : EMPTY;
            uint32_t a = 0;
            bool cand = false;
            if (s < CAP) {
                a = ua[s];
                cand = uplay(uc[s]) == p && (a & UA_DEC) && !(a & (UA_PRESENT | UA_BAD));
            }
            const uint64_t m = ballot(cand);
            if (m == 0) continue;
            const int t = ua_type(a), pr = par[s < CAP ? s : 0];
            int irank = 0;
            const uint64_t acc = acceptChain(p, run0, run1, cand, cand ? lanes_below(m) : -1, __popcll(m), t, pr, c, a, false, irank);
            if ((acc >> lid()) & 1ull) ua[s] = a | UA_PA;
            wsync();
        }
    }
    // Unit-parallel form (all units in one wave): the candidates' ascending-cell order is a rank
    // computed in registers, so the serial part is the acceptance chain alone.
    DEV void decodeUnits(int p, int& run0, int& run1, bool keepBits, bool issueNow) {
        const int o = lid();
        uint32_t a = 0, cu = 0;
        bool cand = false;
        if (o < nu) {
            cu = uc[o];
            a = ua[o];
            cand = !(cu & UC_DEAD) && uplay(cu) == p && (a & UA_DEC) && !(a & (UA_PRESENT | UA_BAD));
        }
        const uint64_t m = ballot(cand);
        if (m == 0) {
            if (issueNow) {
                curP = p;
                issueFills(p, 1);
            }
            return;
        }
        const int c = uy(cu) * W + ux(cu);
        const int pr = o < nu ? par[o] : 0;
        MPHASE(12);
        const int rank = cellRank(m, cand, c);
        MPHASE(14);
        int irank = 0;
        const uint64_t acc = acceptChain(p, run0, run1, cand, rank, __popcll(m), ua_type(a), pr, c, a, keepBits, irank);
        const bool isPA = (acc >> o) & 1ull;
        if (!issueNow) {
            if (isPA) ua[o] = a | UA_PA;
            wsync();
            return;
        }
        MPHASE(2);
        // issuePlayer(p, 1, false) of the accepted lanes (issuePA's legality + issueBatch, then the fills)
        curP = p;
        int t = 0, prm = 0, tx = 0, ty = 0, ut = 0;
        if (isPA) {
            t = ua_type(a);
            prm = pr;
            tx = ua_tx(a);
            ty = ua_ty(a);
            ut = ua_ut(a);
            // forwarded fused-policy rows (every decoded row here when fwdOn: all units in one wave)
            // are members of getUnitActions' list — see selfPlayFast; the masks, and so the rows,
            // come from the full state in partially observable games too (JNIGridnetClient.java:210-223)
            if (!fwdOn) legality(o, t, prm, tx, ty, ut);
        }
        wsync();
        if (acc) issueBatch(isPA, irank, __popcll(acc), o, t, prm, tx, ty, ut);
        issueFills(p, 1);
    }
    // rank of each candidate lane among the candidates m by cell c (cells are distinct)
    DEV int cellRank(uint64_t m, bool cand, int c) const {
        int rank = 0;
        for (uint64_t mm = m; mm; mm &= mm - 1) rank += rl(c, __builtin_ctzll(mm)) < c;
        return cand ? rank : -1;
    }
    // acceptChain with the reservation bitmap held one word per lane (readlane instead of LDS reads).
    // The candidates' (usesPos, cost, position) keys are first permuted into rank order (lane r holds
    // rank r's key, via rseq), so each chain step is one readlane and a few scalar tests.  The other
    // player's running sum cannot change during p's chain: if it blocks (ResourceUsage.java:38-46),
    // every candidate is rejected.
    DEV uint64_t acceptChainReg(int p, int& run0, int& run1, int rank, int n, bool usesPos, int tpos, int cost, int NB,
                                bool keepBits, int& irank, uint32_t* RB) {
        const int l = lid();
        {
            // Parallel form for the common case: when no candidate's used position is reserved already,
            // no two candidates use the same position, and the base reservations plus every candidate's
            // cost fit the player's resources, each sequential consistentWith test below passes (the
            // running sum only grows by accepted costs, so every prefix fits too) — accept them all.
            const int runQ = p == 0 ? run1 : run0, presQ = p == 0 ? pres1 : pres0, presP = p == 0 ? pres0 : pres1;
            const int runP = p == 0 ? run0 : run1;
            const bool cand = rank >= 0, up = cand && usesPos;
            if (!(runQ != 0 && runQ > 0 && runQ > presQ)) {
                bool conf = false;
                // reserved already, or used by another candidate: each candidate ORs its position into a
                // copy of the reservation words (rseq, free here) and is in conflict when the bit was set —
                // by the base reservations or by another candidate (one of each equal pair sees it; round 5,
                // in place of a readlane walk over the candidates)
                uint32_t* cp = (uint32_t*)rseq;
                if (l < NB) cp[l] = RB[l];
                wsync();
                if (up) conf = (atomicOr(&cp[tpos >> 5], 1u << (tpos & 31)) >> (tpos & 31)) & 1u;
                wsync();
                int sumc = 0;
                if (walk) {  // the candidates' PRODUCE costs (a few lanes): one lane read each
                    for (uint64_t mm = ballot(cand && cost > 0); mm; mm &= mm - 1) sumc += uni(rl(cost, __builtin_ctzll(mm)));
                } else if (ballot(cand && cost > 0)) {
                    sumc = wave_sum(cand ? cost : 0);
                }
                if (!ballot(conf) && runP + sumc <= presP) {
                    if (p == 0) run0 = runP + sumc;
                    else run1 = runP + sumc;
                    if (!keepBits && up) atomicOr(&RB[tpos >> 5], 1u << (tpos & 31));
                    if (cand) irank = rank;
                    wsync();
                    return ballot(cand);
                }
            }
        }
        uint32_t bv = l < NB ? RB[l] : 0u;
        if (rank >= 0) rseq[rank] = (int)(((uint32_t)usesPos << 31) | ((uint32_t)cost << 16) | ((uint32_t)tpos & 0xFFFFu));
        wsync();
        const int keyR = l < n ? rseq[l] : 0;
        const int runQ = p == 0 ? run1 : run0, presQ = p == 0 ? pres1 : pres0, presP = p == 0 ? pres0 : pres1;
        int runP = p == 0 ? run0 : run1;
        uint64_t accR = 0;  // accepted, bit r = rank r
        if (!(runQ != 0 && runQ > 0 && runQ > presQ)) {
            for (int r = 0; r < n; r++) {
                const uint32_t key = uniu((uint32_t)rl(keyR, r));
                const int bi = (int)(key & 0xFFFFu), cst = (int)((key >> 16) & 0x7FFFu);
                const bool up = key >> 31;
                bool ok = true;
                if (up) ok = !(((uint32_t)rl((int)bv, bi >> 5) >> (bi & 31)) & 1u);
                if (runP != 0) {
                    const int sum = cst + runP;
                    if (sum > 0 && sum > presP) ok = false;
                }
                if (ok) {
                    if (up && l == (bi >> 5)) bv |= 1u << (bi & 31);
                    runP += cst;
                    accR |= 1ull << r;
                }
            }
        }
        if (p == 0) run0 = runP;
        else run1 = runP;
        wsync();  // rseq is read again by the next chain
        if (!keepBits && l < NB) RB[l] = bv;
        const bool isAcc = rank >= 0 && ((accR >> rank) & 1ull);
        if (isAcc) irank = __popcll(accR & ((1ull << rank) - 1ull));
        return ballot(isAcc);
    }
    // ua.ru.consistentWith(running ru) for the n candidates in rank order (PlayerAction.java:400-415);
    // returns the accepted lanes
    // keepBits: `bits` is left as it was (the chain's additions stay in registers)
    // irank: each accepted lane's rank among the accepted (the pa's issue order)
    DEV uint64_t acceptChain(int p, int& run0, int& run1, bool cand, int rank, int n, int t, int pr, int c, uint32_t a,
                             bool keepBits, int& irank, uint32_t* RB = nullptr) {
        const bool usesPos = cand && (t == T_MOVE || t == T_PRODUCE);
        const int tpos = c + dyo(pr) * W + dxo(pr) + W;  // ResourceUsage position (UnitAction.java:254-291)
        const int cost = (cand && t == T_PRODUCE) ? U.cost[ua_ut(a)] : 0;
        const int NB = (HW + 2 * W + 31) / 32;
        if (NB <= 64) return acceptChainReg(p, run0, run1, rank, n, usesPos, tpos, cost, NB, keepBits, irank, RB ? RB : bits);
        uint64_t acc = 0;
        int nacc = 0;
        for (int r = 0; r < n; r++) {
            const int k = __builtin_ctzll(ballot(rank == r));
            const bool up = rl(usesPos, k);
            const int bi = rl(tpos, k), cst = rl(cost, k);
            bool ok = true;
            if (up) ok = !((uniu(bits[bi >> 5]) >> (bi & 31)) & 1u);
            if (run0 != 0) {
                const int sum = (p == 0 ? cst : 0) + run0;
                if (sum > 0 && sum > pres0) ok = false;
            }
            if (run1 != 0) {
                const int sum = (p == 1 ? cst : 0) + run1;
                if (sum > 0 && sum > pres1) ok = false;
            }
            if (ok) {
                if (up && lid() == 0) bits[bi >> 5] |= 1u << (bi & 31);
                if (p == 0) run0 += cst;
                else run1 += cst;
                acc |= 1ull << k;
                if (lid() == k) irank = nacc;
                nacc++;
            }
        }
        return acc;
    }

    // ------------------------------------------------------------------ issueSafe / issue
    // Unit.canExecuteAction (rts/units/Unit.java:531-534) = membership in getUnitActions
    // (:382-522) under UnitAction.equals (rts/UnitAction.java:191-208); an illegal action becomes
    // NONE(ETA(original)) (rts/GameState.java:347-354).  Lane-local.
    DEV void legality(int s, int& t, int& prm, int& tx, int& ty, int& ut) const { legality(s, uc[s], t, prm, tx, ty, ut); }
    DEV void legality(int s, uint32_t cu, int& t, int& prm, int& tx, int& ty, int& ut) const {
        const int x = ux(cu), y = uy(cu), typ = utyp(cu), pl = uplay(cu);
        const uint32_t fl = U.flags[typ];
        bool legal = false;
        int etaOrig = 0;
        switch (t) {
            case T_NONE: legal = true; break;
            case T_MOVE:
                etaOrig = U.moveT[typ];
                if ((fl & F_MOVE) && prm < 4) {
                    const int nx = x + dxo(prm), ny = y + dyo(prm);
                    legal = inb(nx, ny) && cell[ny * W + nx] == EMPTY;
                }
                break;
            case T_HARVEST:
                etaOrig = U.harvestT[typ];
                if ((fl & F_HARVEST) && res[s] == 0 && prm < 4) {
                    const int nx = x + dxo(prm), ny = y + dyo(prm);
                    if (inb(nx, ny)) {
                        const int n = cell[ny * W + nx];
                        legal = n < CAP && (U.flags[utyp(uc[n])] & F_RESOURCE);
                    }
                }
                break;
            case T_RETURN:
                etaOrig = U.moveT[typ];
                if ((fl & F_HARVEST) && res[s] > 0 && prm < 4) {
                    const int nx = x + dxo(prm), ny = y + dyo(prm);
                    if (inb(nx, ny)) {
                        const int n = cell[ny * W + nx];
                        legal = n < CAP && (U.flags[utyp(uc[n])] & F_STOCKPILE) && uplay(uc[n]) == pl;
                    }
                }
                break;
            case T_PRODUCE: {
                etaOrig = U.produceT[ut];
                bool produces = false;
                for (int i = 0; i < U.nprod[typ]; i++) produces |= (U.prod[typ][i] == ut);
                if (produces && prm < 4 && pres(pl) >= U.cost[ut]) {
                    const int nx = x + dxo(prm), ny = y + dyo(prm);
                    legal = inb(nx, ny) && cell[ny * W + nx] == EMPTY;
                }
            } break;
            case T_ATTACK:
                etaOrig = U.attackT[typ];
                if ((fl & F_ATTACK) && tx != 255) {
                    const int n = cell[ty * W + tx];
                    if (n < CAP) {
                        const int tp = uplay(uc[n]);
                        if (tp >= 0 && tp != pl) {
                            const int dx = tx - x, dy = ty - y, r = U.range[typ];
                            legal = (r == 1) ? (abs(dx) + abs(dy) == 1) : (dx * dx + dy * dy <= r * r);
                        }
                    }
                }
                break;
            default: etaOrig = 0; break;  // unknown type: ETA 0 (UnitAction.java:328)
        }
        if (!legal) {
            t = T_NONE;
            prm = etaOrig;
            tx = ty = ut = 0;
        } else if (t == T_ATTACK) {
            prm = -1;
        }
    }

    // Does present assignment o conflict with a new MOVE/PRODUCE (target ntgt, producer player pl,
    // cost ncost) — !old.ru.consistentWith(new ru) (GameState.java:264, ResourceUsage.java:31-50)
    DEV bool conflicts(int o, int ntgt, bool nProduce, int ncost, int pl) const {
        const uint32_t a = ua[o];
        if (!(a & UA_PRESENT)) return false;
        const int ot = ua_type(a);
        if (ot != T_MOVE && ot != T_PRODUCE) return false;
        const uint32_t oc = uc[o];
        const int od = par[o];
        if (((uy(oc) + dyo(od)) * W + ux(oc) + dxo(od)) == ntgt) return true;
        if (nProduce) {
            const int ores = (ot == T_PRODUCE && uplay(oc) == pl) ? U.cost[ua_ut(a)] : 0;
            const int sum = ores + ncost;
            if (sum > 0 && sum > pres(pl)) return true;
        }
        return false;
    }

    // GameState.issue for one pair (rts/GameState.java:252-326), wave-uniform arguments.  Returns the
    // type of the action put into the map (NONE when a conflict cancelled the new one).
    DEV int issueOne(int s, int t, int prm, int tx, int ty, int ut) {
        if (t == T_MOVE || t == T_PRODUCE) {
            const uint32_t cu = uniu(uc[s]);
            const int pl = uplay(cu), typ = utyp(cu);
            const int ntgt = (uy(cu) + dyo(prm)) * W + ux(cu) + dxo(prm);
            const bool nProduce = (t == T_PRODUCE);
            const int ncost = nProduce ? U.cost[ut] : 0;
            bool any = false;
            for (int o0 = 0; o0 < nu; o0 += 64) {
                const int o = o0 + lid();
                any |= ballot(o < nu && conflicts(o, ntgt, nProduce, ncost, pl)) != 0;
            }
            int lastSeq = -1;
            bool orig = true;  // p still names pa's own Pair (GameState.java:296 replaces only the loop variable)
            const int tIn = t, utIn = ut;
            while (any) {  // rare: resolve the conflicting assignments in insertion order
                int best = INF;
                for (int o = lid(); o < nu; o += 64)
                    if (as[o] > lastSeq && conflicts(o, ntgt, nProduce, ncost, pl)) best = min(best, as[o]);
                best = wave_min(best);
                if (best == INF) break;
                int os = INF;
                for (int o = lid(); o < nu; o += 64)
                    if ((ua[o] & UA_PRESENT) && as[o] == best) os = o;
                os = wave_min(os);
                lastSeq = best;
                if (uni(at[os]) == time) {  // same-cycle conflict: policy (GameState.java:266-297)
                    bool cold = false, cnew = false;
                    if (U.crs == 2) {
                        JRand rc = rngLoad(H_RNG_CANCEL);
                        if (rc.nextInt(2) == 0) cnew = true;
                        else cold = true;
                        rngStore(H_RNG_CANCEL, rc);
                    } else if (U.crs == 3) {
                        const int cc = hget(H_CANCEL_CNT);
                        if ((cc % 2) == 0) cnew = true;
                        else cold = true;
                        hset(H_CANCEL_CNT, cc + 1);
                    } else {
                        cold = cnew = true;
                    }
                    const int d1 = uni(etaSlot(os));
                    const int d2 = eta(t, prm, ut, typ);
                    const int md = min(d1, d2);
                    if (cold) {
                        if (lid() == 0) {
                            ua[os] = pack_ua(T_NONE, 0, 0, 0) | UA_PRESENT;
                            par[os] = (int16_t)md;
                            if (po) {  // the mutated UAA object is shared with the PO snapshots holding it
                                uint32_t b = snap[os];
                                for (int q = 0; q < 2; q++)
                                    if (snap_in(b, q) && snap_act(b, q) && as[os] < hdr[HX_SNAP + q])
                                        b = (b & ~(7u << (2 + 3 * q))) | ((uint32_t)(T_NONE + 1) << (2 + 3 * q));
                                snap[os] = (uint8_t)b;
                            }
                        }
                    }
                    if (cnew) {
                        t = T_NONE;
                        prm = md;
                        tx = ty = ut = 0;
                        orig = false;
                    }
                    wsync();
                } else {  // older assignment: only the new one is cancelled (:298-317)
                    // p.m_b = NONE mutates pa's own Pair unless a cancel already replaced p: the
                    // TraceEntry (pa.clone() after issueSafe) then records NONE, not the PRODUCE
                    if (orig && tIn == T_PRODUCE && (D_ZERO(reward_need) & RN_COUNTS) && lid() == 0) {
                        const int pc = prodCategory(U.flags[utIn]);
                        if (pc >= 0) rwc[curP * RC_N + pc] -= 1;
                    }
                    orig = false;
                    addErr(E_OLDER);
                    t = T_NONE;
                    prm = -1;
                    tx = ty = ut = 0;
                }
            }
        }
        // a unit with an assignment here got it from an earlier pair of this pa (Java rows may name a
        // unit twice): LinkedHashMap.put replaces the value and keeps the entry's position
        const bool again = (uniu(ua[s]) & UA_PRESENT) != 0;
        if (lid() == 0) {
            ua[s] = pack_ua(t, ut, tx, ty) | UA_PRESENT;
            par[s] = (int16_t)prm;
            at[s] = time;
            if (!again) as[s] = seq;
        }
        if (!again) seq++;
        wsync();
        return t;
    }

    // Issue index over ALL units (GameState.issue checks every present assignment, :255-262); under
    // full observability it is also every view's base ResourceUsage (PlayerAction.java:387-394).
    DEV void buildIndex() {
#ifdef MRTS_PHASE_TIMING
#ifndef MRTS_SPAN_ONLY
        phAcc[15] += 1000;  // call counter (x1000 so the per-step mean shows)
#endif
#endif
        const int NB = (HW + 2 * W + 31) / 32;
        for (int i = lid(); i < NB; i += 64) bits[i] = 0;
        wsync();
        bool mp = false;
        if (walk) {
            // the present PRODUCEs' costs per player (largest, sum) by walking their few lanes: one lane read
            // each (cost | player << 16), scalar max / add, instead of four whole-wave reductions
            int mc0 = -1, mc1 = -1, s0 = 0, s1 = 0;
            for (int o0 = 0; o0 < nu; o0 += 64) {
                const int o = o0 + lid();
                int key = -1;
                if (o < nu) {
                    const uint32_t a = ua[o];
                    const int t = ua_type(a);
                    if ((a & UA_PRESENT) && (t == T_MOVE || t == T_PRODUCE)) {
                        mp = true;
                        const uint32_t c = uc[o];
                        const int d = par[o];
                        const int pos = (uy(c) + dyo(d)) * W + ux(c) + dxo(d) + W;
                        atomicOr(&bits[pos >> 5], 1u << (pos & 31));
                        if (t == T_PRODUCE) key = U.cost[ua_ut(a)] | ((uplay(c) == 0 ? 0 : 1) << 16);
                    }
                }
                for (uint64_t mm = ballot(key >= 0); mm; mm &= mm - 1) {
                    const int kv = uni(rl(key, __builtin_ctzll(mm)));
                    const int k = kv & 0xFFFF;
                    if ((kv >> 16) == 0) {
                        mc0 = max(mc0, k);
                        s0 += k;
                    } else {
                        mc1 = max(mc1, k);
                        s1 += k;
                    }
                }
            }
            anyMP = ballot(mp) != 0;
            maxProd0 = mc0;
            maxProd1 = mc1;
            sumProd0 = s0;
            sumProd1 = s1;
        } else {
            int mc0 = -1, mc1 = -1, s0 = 0, s1 = 0;
            for (int o = lid(); o < nu; o += 64) {
                const uint32_t a = ua[o];
                const int t = ua_type(a);
                if (!(a & UA_PRESENT) || (t != T_MOVE && t != T_PRODUCE)) continue;
                mp = true;
                const uint32_t c = uc[o];
                const int d = par[o];
                const int pos = (uy(c) + dyo(d)) * W + ux(c) + dxo(d) + W;
                atomicOr(&bits[pos >> 5], 1u << (pos & 31));
                if (t == T_PRODUCE) {
                    const int k = U.cost[ua_ut(a)];
                    if (uplay(c) == 0) {
                        mc0 = max(mc0, k);
                        s0 += k;
                    } else {
                        mc1 = max(mc1, k);
                        s1 += k;
                    }
                }
            }
            anyMP = ballot(mp) != 0;
            if (ballot(mc0 >= 0 || mc1 >= 0)) {  // any present PRODUCE (rare)
                maxProd0 = -wave_min(-mc0);
                maxProd1 = -wave_min(-mc1);
                sumProd0 = wave_sum(s0);
                sumProd1 = wave_sum(s1);
            } else {
                maxProd0 = maxProd1 = -1;
                sumProd0 = sumProd1 = 0;
            }
        }
        ixValid = true;
        if (steady) prodDirty = false;
        wsync();
    }
    // The steady instance's step start in place of buildIndex: the index the previous step of this
    // launch left is still the state's.  Between a step's issue pass (which keeps the index: issueBothWrite,
    // issueBatch) and the next one only cycleLanes (the ready assignments), kill (a dead unit's; cycleLanes' last lines) and
    // resetFromTemplate remove assignments; the first two give the position back — no two present assignments
    // share one (GameState.issue, rts/GameState.java:252-326: the acceptance chain, issueBothTest and issueBatch
    // enforce it) — the third, and every path that leaves the lane-parallel ones, clears ixValid.  Left here: the
    // PRODUCE costs when one of them went.  anyMP is not carried: issueBatch, its one reader, takes it from `bits`.
    DEV void carryIndex() {
        if (MRTS_UNLIKELY(prodDirty)) {
            const bool np = lid() < nu && (lua & UA_PRESENT) && ua_type(lua) == T_PRODUCE;
            int s0 = 0, s1 = 0, mc0 = -1, mc1 = -1;
            prodCosts(np, np ? U.cost[ua_ut(lua)] : 0, uplay(lcu) == 0 ? 0 : 1, s0, s1, mc0, mc1);
            sumProd0 = s0;
            sumProd1 = s1;
            maxProd0 = mc0;
            maxProd1 = mc1;
            prodDirty = false;
        }
#ifdef MRTS_LANE_AUDIT
        auditIndex();
#endif
    }
#ifdef MRTS_LANE_AUDIT
    // audit build: the index built the old way into scratch (`rseq`, free at the step's start) against the carried one
    DEV void auditIndex() {
        const int NB = (HW + 2 * W + 31) / 32;  // <= 64 (useIx)
        const int l = lid();
        uint32_t* const sb = (uint32_t*)rseq;
        wsync();
        if (l < NB) sb[l] = 0;
        wsync();
        int key = -1;
        if (l < nu) {
            const uint32_t a = ua[l];
            const int t = ua_type(a);
            if ((a & UA_PRESENT) && (t == T_MOVE || t == T_PRODUCE)) {
                const uint32_t c = uc[l];
                const int d = par[l];
                const int pos = (uy(c) + dyo(d)) * W + ux(c) + dxo(d) + W;
                atomicOr(&sb[pos >> 5], 1u << (pos & 31));
                if (t == T_PRODUCE) key = U.cost[ua_ut(a)] | ((uplay(c) == 0 ? 0 : 1) << 16);
            }
        }
        wsync();
        const int k = key & 0xFFFF;
        const bool p0 = key >= 0 && (key >> 16) == 0, p1 = key >= 0 && (key >> 16) == 1;
        const int s0 = wave_sum(p0 ? k : 0), s1 = wave_sum(p1 ? k : 0);
        const int mc0 = -wave_min(p0 ? -k : 1), mc1 = -wave_min(p1 ? -k : 1);
        const bool diff = l < NB && sb[l] != bits[l];
        if (ballot(diff) || s0 != sumProd0 || s1 != sumProd1 || mc0 != maxProd0 || mc1 != maxProd1)
            addErr(E_INDEX);
        wsync();
    }
#endif

    // GameState.issue (rts/GameState.java:252-326) for a batch of (unit s, action) lanes in rank order
    // 0..n-1.  When no new MOVE/PRODUCE conflicts with a present assignment or an earlier one of the
    // batch, every issue() takes its no-conflict branch and the batch is issued in parallel (seq =
    // seq + rank); otherwise the batch runs one pair at a time through issueOne.
    // checkDup (Java rows): a unit named by an earlier pair of this pa (same batch, or already issued)
    // forces the one-at-a-time path
    // cuKnown: the lane's unit core word uc[s] (already in a register), or null
    // putAny (trace replay): set when a pair is put with a type other than NONE — GameState.issue's
    // return value (:323-324)
    // posChecked: the batch's MOVE / PRODUCE positions are known to be distinct and unreserved (the rows
    // passed acceptChain's ResourceUsage test against this same index: selfPlayFast) — the pairwise
    // walk then visits the PRODUCE lanes only, for the cost sums (round 5: it read four values per MOVE
    // lane per batch)
    DEV void issueBatch(bool act, int rank, int n, int s, int t, int prm, int tx, int ty, int ut, bool checkDup = false,
                        const uint32_t* cuKnown = nullptr, bool* putAny = nullptr, bool posChecked = false) {
        const bool mp = act && (t == T_MOVE || t == T_PRODUCE);
        const bool np = act && t == T_PRODUCE;
        if (MRTS_UNLIKELY(D_ZERO(reward_need) & RN_COUNTS)) {  // the pairs as the TraceEntry records them (legality applied)
            const int pc = np ? prodCategory(U.flags[ut]) : -1;
            auto cnt = [](bool b) { return (int)__popcll(ballot(b)); };
            const int c[RC_N] = {cnt(act && t == T_HARVEST), cnt(act && t == T_RETURN), cnt(act && t == T_ATTACK),
                                 cnt(pc == RC_PROD_WORKER), cnt(pc == RC_PROD_BUILDING), cnt(pc == RC_PROD_COMBAT)};
            if (lid() == 0)
#pragma unroll
                for (int k = 0; k < RC_N; k++) rwc[curP * RC_N + k] += c[k];
        }
        const uint64_t mpm = ballot(mp);
        bool conf = false;
        if (checkDup) {
            if (act && (ua[s] & UA_PRESENT)) conf = true;
            for (uint64_t mm = ballot(act); mm; mm &= mm - 1) {
                const int k = __builtin_ctzll(mm);
                const int sk = rl(s, k), rk = rl(rank, k);  // uniform flow (no readlane under a lane test)
                if (act && sk == s && rk < rank) conf = true;
            }
        }
        int ntgt = 0, ncost = 0, pl = 0;
        if (mpm) {
            if (!ixValid) buildIndex();
            // (steady: a carried index brings no anyMP along — any bit of `bits` is a present MOVE / PRODUCE)
            if (steady && ballot(np)) anyMP = ballot(lid() < (HW + 2 * W + 31) / 32 && bits[lid()] != 0) != 0;
            if (mp) {
                const uint32_t cu = cuKnown ? *cuKnown : uc[s];
                pl = uplay(cu);
                ntgt = (uy(cu) + dyo(prm)) * W + ux(cu) + dxo(prm);
                ncost = np ? U.cost[ut] : 0;
                const int pr = pl == 0 ? pres0 : pres1;
                if ((bits[(ntgt + W) >> 5] >> ((ntgt + W) & 31)) & 1u) conf = true;
                if (np) {
                    if (anyMP && ncost > 0 && ncost > pr) conf = true;
                    const int mc = pl == 0 ? maxProd0 : maxProd1;
                    if (mc >= 0 && mc + ncost > 0 && mc + ncost > pr) conf = true;
                }
            }
            if (posChecked && ballot(np && ncost > 0 && ncost > (pl == 0 ? pres0 : pres1))) {
                // a PRODUCE whose cost alone exceeds the resources conflicts with any earlier MOVE / PRODUCE
                // of the batch (consistentWith: 0 + cost > resources) — the walk below skips the MOVEs
                const int minRank = wave_min(mp ? rank : INF);
                if (np && ncost > 0 && ncost > (pl == 0 ? pres0 : pres1) && minRank < rank) conf = true;
            }
            for (uint64_t mm = posChecked ? ballot(np) : mpm; mm; mm &= mm - 1) {  // earlier MOVE/PRODUCE lanes of the batch
                const int k = __builtin_ctzll(mm);
                const int rk = rl(rank, k), tk = posChecked ? 0 : rl(ntgt, k), pk = rl(pl, k), ck = rl(np ? ncost : -1, k);
                if (mp && rk < rank) {
                    if (!posChecked && tk == ntgt) conf = true;
                    if (np) {
                        const int sum = ((ck >= 0 && pk == pl) ? ck : 0) + ncost;
                        if (sum > 0 && sum > (pl == 0 ? pres0 : pres1)) conf = true;
                    }
                }
            }
        }
        if (MRTS_LIKELY(ballot(conf) == 0)) {
            if (putAny && ballot(act && t != T_NONE)) *putAny = true;
            if (act) {
                ua[s] = pack_ua(t, ut, tx, ty) | UA_PRESENT;
                par[s] = (int16_t)prm;
                at[s] = time;
                as[s] = seq + rank;
                if (mp && ixValid) atomicOr(&bits[(ntgt + W) >> 5], 1u << ((ntgt + W) & 31));
            }
            seq += n;
            if (mpm) {
                anyMP = true;
                if (walk) {
                    // the batch's PRODUCEs (a few lanes): one lane read each, scalar max / add
                    for (uint64_t mm = ballot(np); mm; mm &= mm - 1) {
                        const int kv = uni(rl(ncost | (pl << 16), __builtin_ctzll(mm)));
                        const int k = kv & 0xFFFF;
                        if ((kv >> 16) == 0) {
                            maxProd0 = max(maxProd0, k);
                            sumProd0 += k;
                        } else if ((kv >> 16) == 1) {
                            maxProd1 = max(maxProd1, k);
                            sumProd1 += k;
                        }
                    }
                } else {
                    if (ballot(np)) {  // PRODUCE is rare: skip the four reductions otherwise
                        maxProd0 = max(maxProd0, -wave_min(np && pl == 0 ? -ncost : 1));
                        maxProd1 = max(maxProd1, -wave_min(np && pl == 1 ? -ncost : 1));
                        sumProd0 += wave_sum(np && pl == 0 ? ncost : 0);
                        sumProd1 += wave_sum(np && pl == 1 ? ncost : 0);
                    }
                }
            }
            wsync();
        } else {
#ifdef MRTS_PHASE_TIMING
#ifndef MRTS_SPAN_ONLY
            phAcc[11] += 1000;  // slow-path batches
#endif
#endif
            for (int r = 0; r < n; r++) {
                const int k = __builtin_ctzll(ballot(act && rank == r));
                const int put = issueOne(rl(s, k), rl(t, k), rl(prm, k), rl(tx, k), rl(ty, k), rl(ut, k));
                if (putAny && put != T_NONE) *putAny = true;
            }
            ixValid = false;
        }
    }

    // GameState.issueSafe(pa) (rts/GameState.java:338-408) of the lanes' decoded actions.
    DEV void issuePA(int s, bool isPA, int rank, int n) {
        int t = 0, prm = 0, tx = 0, ty = 0, ut = 0;
        if (isPA) {
            const uint32_t a = ua[s];
            t = ua_type(a);
            prm = par[s];
            tx = ua_tx(a);
            ty = ua_ty(a);
            ut = ua_ut(a);
            legality(s, t, prm, tx, ty, ut);
        }
        wsync();
        issueBatch(isPA, rank, n, s, t, prm, tx, ty, ut);
    }
    // Agent pa = [accepted rows in cell order] + PlayerAction.fillWithNones(gs, p, fillDur)
    // (rts/PlayerAction.java:217-235) in list order; AI pa (RandomBiasedAI / PassiveAI) = its units
    // in list order (listOrder).
    DEV void issuePlayer(int p, int fillDur, bool listOrder) {
        curP = p;
        if (!listOrder && nu <= 64) {
            const int o = lid();
            uint32_t cu = 0;
            bool isPA = false;
            if (o < nu) {
                cu = uc[o];
                isPA = !(cu & UC_DEAD) && uplay(cu) == p && (ua[o] & UA_PA);
            }
            const uint64_t m = ballot(isPA);
            if (m) issuePA(o, isPA, cellRank(m, isPA, uy(cu) * W + ux(cu)), __popcll(m));
        } else if (!listOrder) {
            for (int c0 = 0; c0 < HW; c0 += 64) {
                const int c = c0 + lid();
                const int s = c < HW ? cell[c] : EMPTY;
                const bool isPA = s < CAP && uplay(uc[s]) == p && (ua[s] & UA_PA);
                const uint64_t m = ballot(isPA);
                if (m) issuePA(s, isPA, lanes_below(m), __popcll(m));
            }
        } else {
            for (int o0 = 0; o0 < nu; o0 += 64) {
                const int o = o0 + lid();
                const bool isPA = o < nu && !(uc[o] & UC_DEAD) && uplay(uc[o]) == p && (ua[o] & UA_PA);
                const uint64_t m = ballot(isPA);
                if (m) issuePA(o, isPA, lanes_below(m), __popcll(m));
            }
        }
        issueFills(p, fillDur);
    }
    // the NONE fills never conflict (issue() checks MOVE/PRODUCE only): parallel, seq in list order
    DEV void issueFills(int p, int fillDur) {
        for (int o0 = 0; o0 < nu; o0 += 64) {
            const int o = o0 + lid();
            bool fill = false;
            if (o < nu) {
                const uint32_t c = uc[o];
                fill = !(c & UC_DEAD) && uplay(c) == p && !(ua[o] & (UA_PRESENT | UA_PA));
            }
            const uint64_t m = ballot(fill);
            if (fill) {
                ua[o] = pack_ua(T_NONE, 0, 0, 0) | UA_PRESENT;
                par[o] = (int16_t)fillDur;
                at[o] = time;
                as[o] = seq + lanes_below(m);
            }
            seq += __popcll(m);
        }
        wsync();
    }

    // ------------------------------------------------------------------ RandomBiasedAI
    // RandomBiasedAI.getAction (ai/RandomBiasedAI.java:51-107): for every idle unit of b in list
    // order, getUnitActions(gs) (rts/units/Unit.java:382-522) weighted 5 (attack/harvest/return) or 1,
    // Sampler.weighted (util/Sampler.java:116-135) with the game's java.util.Random, then accepted iff
    // consistent with the running reservations, else that list's NONE(10).  The chosen actions are
    // parked with UA_PA and issued later in list order.  getUnitActions of an owned unit is the same
    // in every view (neighbours and range-3 targets are always inside its own sight radius), the
    // base reservations are the view's (PO: b's snapshot).
    DEV void randomBiased(int b) {
        bool anyIdle = false;
        for (int o0 = 0; o0 < nu; o0 += 64) {
            const int o = o0 + lid();
            anyIdle |= ballot(o < nu && !(uc[o] & UC_DEAD) && uplay(uc[o]) == b && !(ua[o] & UA_PRESENT)) != 0;
        }
        if (!anyIdle) return;  // canExecuteAnyAction (rts/GameState.java:416-423): empty pa, no draws
        int run0, run1;
        baseReservations(b, run0, run1);
        for (int o0 = 0; o0 < nu; o0 += 64) {
            const int o = o0 + lid();
            uint64_t m = ballot(o < nu && !(uc[o] & UC_DEAD) && uplay(uc[o]) == b && !(ua[o] & UA_PRESENT));
            while (m) {
                const int k = __builtin_ctzll(m);
                m &= m - 1;
                pickRandomBiased(o0 + k, b, run0, run1);
            }
        }
    }
    DEV void pickRandomBiased(int s, int b, int& run0, int& run1) {
        const uint32_t cu = uniu(uc[s]);
        const int x = ux(cu), y = uy(cu), typ = utyp(cu);
        const uint32_t fl = U.flags[typ];
        const int carried = uni(res[s]);
        int nb[4];
        uint32_t atkDirs = 0, harvDirs = 0, retDirs = 0, freeDirs = 0;
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const int nx = x + dxo(d), ny = y + dyo(d);
            nb[d] = inb(nx, ny) ? uni(cell[ny * W + nx]) : WALL;
            if (nb[d] < CAP) {
                const uint32_t oc = uniu(uc[nb[d]]);
                const int op = uplay(oc);
                const uint32_t ofl = U.flags[utyp(oc)];
                if (op >= 0 && op != b) atkDirs |= 1u << d;
                if (ofl & F_RESOURCE) harvDirs |= 1u << d;
                if ((ofl & F_STOCKPILE) && op == b) retDirs |= 1u << d;
            } else if (nb[d] == EMPTY) {
                freeDirs |= 1u << d;
            }
        }
        const int r = U.range[typ];
        int nAtk = 0;
        if (fl & F_ATTACK) {
            if (r == 1) {
                nAtk = __popc(atkDirs);
            } else {
                for (int q0 = 0; q0 < nu; q0 += 64) {
                    const int q = q0 + lid();
                    bool in = false;
                    if (q < nu) {
                        const uint32_t qc = uc[q];
                        const int op = uplay(qc), dx = ux(qc) - x, dy = uy(qc) - y;
                        in = !(qc & UC_DEAD) && op >= 0 && op != b && dx * dx + dy * dy <= r * r;
                    }
                    nAtk += __popcll(ballot(in));
                }
            }
        }
        const int nHarv = (fl & F_HARVEST) && carried == 0 ? __popc(harvDirs) : 0;
        const int nRet = (fl & F_HARVEST) && carried > 0 ? __popc(retDirs) : 0;
        int nProd = 0;
        for (int i = 0; i < U.nprod[typ]; i++)
            if (pres(b) >= U.cost[U.prod[typ][i]]) nProd += __popc(freeDirs);
        const int nMove = (fl & F_MOVE) ? __popc(freeDirs) : 0;
        const int n5 = nAtk + nHarv + nRet, n1 = nProd + nMove + 1;
        double total = 0.0;
        for (int i = 0; i < n5; i++) total += 5.0;
        for (int i = 0; i < n1; i++) total += 1.0;
        JRand rs = rngLoad(H_RNG_SAMPLER);
        const double tmp = rs.nextDouble() * total;
        rngStore(H_RNG_SAMPLER, rs);
        int idx = -1;
        double accum = 0.0;
        for (int i = 0; i < n5 + n1; i++) {
            accum += i < n5 ? 5.0 : 1.0;
            if (accum >= tmp) {
                idx = i;
                break;
            }
        }
        auto nth = [](uint32_t m, int n) {  // n-th set bit (0-based)
            for (int i = 0; i < n; i++) m &= m - 1;
            return __builtin_ctz(m);
        };
        int t = T_NONE, prm = 10, ut = 0, tx = 0, ty = 0;
        if (idx < nAtk) {
            t = T_ATTACK;
            prm = -1;
            if (r == 1) {
                const int d = nth(atkDirs, idx);
                tx = x + dxo(d);
                ty = y + dyo(d);
            } else {  // idx-th enemy in list order inside the disk
                int seen = 0;
                for (int q0 = 0; q0 < nu; q0 += 64) {
                    const int q = q0 + lid();
                    uint32_t qc = 0;
                    bool in = false;
                    if (q < nu) {
                        qc = uc[q];
                        const int op = uplay(qc), dx = ux(qc) - x, dy = uy(qc) - y;
                        in = !(qc & UC_DEAD) && op >= 0 && op != b && dx * dx + dy * dy <= r * r;
                    }
                    const uint64_t mm = ballot(in);
                    const int cnt = __popcll(mm);
                    if (idx - seen < cnt) {
                        uint64_t z = mm;
                        for (int i = 0; i < idx - seen; i++) z &= z - 1;
                        const uint32_t tc = (uint32_t)rl((int)qc, __builtin_ctzll(z));
                        tx = ux(tc);
                        ty = uy(tc);
                        break;
                    }
                    seen += cnt;
                }
            }
        } else if (idx < nAtk + nHarv) {
            t = T_HARVEST;
            prm = nth(harvDirs, idx - nAtk);
        } else if (idx < n5) {
            t = T_RETURN;
            prm = nth(retDirs, idx - nAtk - nHarv);
        } else {
            int j = idx - n5;
            if (j < nProd) {
                for (int i = 0; i < U.nprod[typ]; i++) {
                    const int u2 = U.prod[typ][i];
                    if (pres(b) < U.cost[u2]) continue;
                    const int n = __popc(freeDirs);
                    if (j < n) {
                        t = T_PRODUCE;
                        ut = u2;
                        prm = nth(freeDirs, j);
                        break;
                    }
                    j -= n;
                }
            } else if (j < nProd + nMove) {
                t = T_MOVE;
                prm = nth(freeDirs, j - nProd);
            }
        }
        // ua.resourceUsage(u, pgs).consistentWith(pa.r, gs) (RandomBiasedAI.java:91)
        bool ok = true;
        int bi = 0, cst = 0;
        const bool up = (t == T_MOVE || t == T_PRODUCE);
        if (up) {
            bi = (y + dyo(prm)) * W + x + dxo(prm) + W;
            ok = !((uniu(bits[bi >> 5]) >> (bi & 31)) & 1u);
        }
        if (t == T_PRODUCE) cst = U.cost[ut];
        if (run0 != 0) {
            const int sum = (b == 0 ? cst : 0) + run0;
            if (sum > 0 && sum > pres0) ok = false;
        }
        if (run1 != 0) {
            const int sum = (b == 1 ? cst : 0) + run1;
            if (sum > 0 && sum > pres1) ok = false;
        }
        if (ok) {
            if (up && lid() == 0) bits[bi >> 5] |= 1u << (bi & 31);
            if (b == 0) run0 += cst;
            else run1 += cst;
        } else {
            t = T_NONE;
            prm = 10;
            ut = tx = ty = 0;
        }
        if (lid() == 0) {
            ua[s] = pack_ua(t, ut, tx, ty) | UA_PA;
            par[s] = (int16_t)prm;
        }
        wsync();
    }

    // ------------------------------------------------------------------ PO snapshot
    // new PartiallyObservableGameState(gs, p) (rts/PartiallyObservableGameState.java:35-54):
    // the list keeps p's units and every other unit whose cell p observes (`observable`, :61-71); the
    // assignment map is the live one at this moment (UAA objects shared).
    // Sight disks (dx^2 + dy^2 <= sightRadius^2 of the seeing unit's type) painted into per-row bitmaps:
    // lane = seeing unit, one atomicOr per covered row word; a cell is seen iff its bit is set.
    DEV void paintDisk(uint32_t* rows, uint32_t u) const {
        const int t = utyp(u);
        paintDiskRows(rows, H, W, ux(u), uy(u), U.sight[t], U.diskLo[t], U.diskHi[t]);
    }
    // paintDisk for every lane with act0 or act1 at once, maps with W <= 32 (one row word) and sight
    // <= 15: a uniform loop over dy up to the table's largest sight, one predicated atomicOr per row
    // and view.  Two views at once: the same disk (same unit) ORed into view 0's rows when act0 and
    // into view 1's when act1 (row buffers rows0 / rows1 chosen per lane).
    DEV void paintDisks2(bool act0, uint32_t* rows0, bool act1, uint32_t* rows1, uint32_t u) const {
        const bool act = act0 || act1;
        const int t = utyp(u), x = ux(u), y = uy(u);
        const int sr = act ? U.sight[t] : -1, SM = U.maxSight;
        const uint32_t dlo = act ? U.diskLo[t] : 0u, dhi = act ? U.diskHi[t] : 0u;
        for (int dy = -SM; dy <= SM; dy++) {
            const int yy = y + dy, ady = dy < 0 ? -dy : dy;
            const int w = (int)(((ady < 8 ? dlo : dhi) >> (4 * (ady & 7))) & 0xFu);
            const int x0 = max(0, x - w), x1 = min(W - 1, x + w);
            const uint32_t b = ((2u << (x1 - x0)) - 1u) << x0;  // columns x0..x1 (x1 - x0 = 31: 2u << 31 wraps to 0)
            const bool row = ady <= sr && yy >= 0 && yy < H;
            if (row && act0) atomicOr(&rows0[yy], b);
            if (row && act1) atomicOr(&rows1[yy], b);
        }
    }
    // one view (the second view's arm folds away)
    DEV void paintDisks(bool act, uint32_t u, uint32_t* rows) const { paintDisks2(act, rows, false, rows, u); }
    DEV bool seen(const uint32_t* rows, int x, int y) const {
        const int WPR = (W + 31) >> 5;
        return (rows[y * WPR + (x >> 5)] >> (x & 31)) & 1u;
    }
    // PartiallyObservableGameState (rts/PartiallyObservableGameState.java:35-71): the view keeps the
    // units inside the sight of player p's (live) units, with the assignments they hold now.  Lane =
    // unit, a uniform loop over the observers (few; painting disks costs more here).
    DEV void snapshot(int p) {
        AB_ON(AB_PO_NOSNAPSHOT, return);
        for (int o0 = 0; o0 < nu; o0 += 64) {
            const int o = o0 + lid();
            uint32_t cu = 0;
            bool live = false;
            if (o < nu) {
                cu = uc[o];
                live = !(cu & UC_DEAD);
            }
            bool vis = live && uplay(cu) == p;
            const int x = ux(cu), y = uy(cu);
            for (int q0 = 0; q0 < nu; q0 += 64) {
                const int q = q0 + lid();
                uint32_t qc = q < nu ? uc[q] : UC_DEAD;
                const bool obs = !(qc & UC_DEAD) && uplay(qc) == p;
                // each observer's x | y << 8 | sight^2 << 16, looked up once per lane, so the serial
                // loop below is one readlane per observer (no dependent LDS read of the sight table)
                const int sr = obs ? U.sight[utyp(qc)] : 0;
                const uint32_t ow = (uint32_t)ux(qc) | ((uint32_t)uy(qc) << 8) | ((uint32_t)(sr * sr) << 16);
                uint64_t m = ballot(obs);
                // two observers per round: independent readlane -> test chains (the loop is latency-bound)
                while (m) {
                    const int k1 = __builtin_ctzll(m);
                    m &= m - 1;
                    const int k2 = m ? __builtin_ctzll(m) : k1;
                    m &= m ? m - 1 : 0ull;
                    const uint32_t w1 = (uint32_t)rl((int)ow, k1), w2 = (uint32_t)rl((int)ow, k2);
                    const int dx1 = (int)(w1 & 0xFFu) - x, dy1 = (int)((w1 >> 8) & 0xFFu) - y;
                    const int dx2 = (int)(w2 & 0xFFu) - x, dy2 = (int)((w2 >> 8) & 0xFFu) - y;
                    vis |= (dx1 * dx1 + dy1 * dy1 <= (int)(w1 >> 16)) | (dx2 * dx2 + dy2 * dy2 <= (int)(w2 >> 16));
                }
            }
            if (o < nu) {
                uint32_t b = snap[o] & ~(1u << p) & ~(7u << (2 + 3 * p));
                if (live && vis) {
                    b |= 1u << p;
                    const uint32_t a = ua[o];
                    if (a & UA_PRESENT) b |= (uint32_t)(ua_type(a) + 1) << (2 + 3 * p);
                }
                snap[o] = (uint8_t)b;
            }
        }
        hset(HX_SNAP + p, seq);
        wsync();
    }
    // Both views' membership at once (self-play, poFast2 shapes): lane = unit paints its sight disk
    // into its own player's row bitmap (the host table's half-widths: the cells dx^2 + dy^2 <= sight^2,
    // exactly snapshot()'s test), then a unit is in view p iff it is live and its cell's bit is set
    // in p's rows (own units cover their own cell).  View 0's assignment bits are taken now; view 1's
    // by snapshotActions(1) after player 0's pairs are issued (the views' unitActions copies are taken
    // at different times; positions and liveness do not change in between).  `vis` is scratch here
    // (the render clears it).
    DEV bool snapBothOk() const { return W <= 32 && H <= 32 && nu <= 64 && U.maxSight <= 15; }
    DEV void snapshotBoth() {
        AB_ON(AB_PO_NOSNAPSHOT, return);
        const int l = lid();
        uint32_t* const r0 = vis;
        uint32_t* const r1 = vis + H;
        if (l < 2 * H) vis[l] = 0;
        const bool inList = l < nu;
        const uint32_t cu = inList ? uc[l] : UC_DEAD;
        const bool live = !(cu & UC_DEAD);
        const int own = uplay(cu);
        wsync();
        paintDisks2(live && own == 0, r0, live && own == 1, r1, cu);
        wsync();
        if (inList) {
            const int x = ux(cu), y = uy(cu);
            const bool in0 = live && ((r0[y] >> x) & 1u), in1 = live && ((r1[y] >> x) & 1u);
            uint32_t b = (in0 ? 1u : 0u) | (in1 ? 2u : 0u);
            const uint32_t a = ua[l];
            if (in0 && (a & UA_PRESENT)) b |= (uint32_t)(ua_type(a) + 1) << 2;
            snap[l] = (uint8_t)b;
        }
        hset(HX_SNAP + 0, seq);
        wsync();
    }
    DEV void snapshotActions(int p) {  // view p's assignment bits now (membership from snapshotBoth)
        AB_ON(AB_PO_NOSNAPSHOT, return);
        const int l = lid();
        if (l < nu) {
            uint32_t b = snap[l] & ~(7u << (2 + 3 * p));
            const uint32_t a = ua[l];
            if (((b >> p) & 1u) && (a & UA_PRESENT)) b |= (uint32_t)(ua_type(a) + 1) << (2 + 3 * p);
            snap[l] = (uint8_t)b;
        }
        hset(HX_SNAP + p, seq);
        wsync();
    }
    DEV void clearSnap() {
        for (int o = lid(); o < CAP; o += 64) snap[o] = 0;
        wsync();
    }

    // ------------------------------------------------------------------ cycle
    DEV void kill(int k) {  // GameState.removeUnit (rts/GameState.java:79-82)
        killedLanes |= ballot(readySlot == k);
        if (lid() == 0) {
            const uint32_t c = uc[k];
            uc[k] = c | UC_DEAD;
            cell[uy(c) * W + ux(c)] = EMPTY;
            ua[k] &= ~UA_PRESENT;
        }
        deaths++;
        wsync();
    }
    // UnitAction.execute (rts/UnitAction.java:338-465) — also for units killed earlier in the loop
    DEV void execute(int s) { execute(s, uniu(uc[s]), uniu(ua[s]), uni(par[s])); }
    // cu / a / prm: the unit's core word, its assignment and parameter (wave-uniform)
    DEV void execute(int s, uint32_t cu, uint32_t a, int prm) {
        const bool dead = cu & UC_DEAD;
        const int x = ux(cu), y = uy(cu), typ = utyp(cu), pl = uplay(cu);
        const int t = ua_type(a);
        switch (t) {
            case T_MOVE: {
                const int nx = x + dxo(prm), ny = y + dyo(prm);
                if (!dead) {
                    if (uni(cell[ny * W + nx]) != EMPTY) addErr(E_COLLISION);
                    if (lid() == 0) {
                        cell[y * W + x] = EMPTY;
                        cell[ny * W + nx] = (uint16_t)s;
                    }
                }
                if (lid() == 0) uc[s] = (cu & ~0xFFFFu) | (uint32_t)nx | ((uint32_t)ny << 8);
                wsync();
            } break;
            case T_ATTACK: {
                const int n = uni(cell[ua_ty(a) * W + ua_tx(a)]);
                if (n < CAP) {
                    int dmg = U.minD[typ];
                    if (U.minD[typ] != U.maxD[typ]) {
                        JRand rd = rngLoad(H_RNG_DAMAGE);
                        dmg = U.minD[typ] + rd.nextInt(1 + (U.maxD[typ] - U.minD[typ]));
                        rngStore(H_RNG_DAMAGE, rd);
                    }
                    const int nhp = uni(hp[n]) - dmg;
                    if (lid() == 0) hp[n] = (int16_t)nhp;
                    wsync();
                    if (nhp <= 0) kill(n);
                }
            } break;
            case T_HARVEST: {
                const int nx = x + dxo(prm), ny = y + dyo(prm);
                if (inb(nx, ny)) {
                    const int n = uni(cell[ny * W + nx]);
                    if (n < CAP && (U.flags[utyp(uniu(uc[n]))] & F_RESOURCE) && (U.flags[typ] & F_HARVEST) && uni(res[s]) == 0) {
                        const int nr = uni(res[n]) - U.harvestAmt[typ];
                        if (lid() == 0) {
                            res[n] = (int16_t)nr;
                            res[s] = (int16_t)U.harvestAmt[typ];
                        }
                        wsync();
                        if (nr <= 0) kill(n);
                    }
                }
            } break;
            case T_RETURN: {
                const int nx = x + dxo(prm), ny = y + dyo(prm);
                if (inb(nx, ny)) {
                    const int n = uni(cell[ny * W + nx]);
                    const int carried = uni(res[s]);
                    if (n < CAP && (U.flags[utyp(uniu(uc[n]))] & F_STOCKPILE) && carried > 0) {
                        addPres(pl, carried);
                        if (lid() == 0) res[s] = 0;
                        wsync();
                    }
                }
            } break;
            case T_PRODUCE: {
                const int ut = ua_ut(a);
                const int nx = x + dxo(prm), ny = y + dyo(prm);
                if (pres(pl) - U.cost[ut] >= 0) {
                    if (uni(cell[ny * W + nx]) != EMPTY) {
                        addErr(E_ADDUNIT);  // PhysicalGameState.addUnit throws (:190-195)
                    } else if (nu >= CAP) {
                        addErr(E_CAPACITY);
                    } else {
                        if (lid() == 0) {
                            uc[nu] = pack_uc(nx, ny, ut, pl);
                            hp[nu] = (int16_t)U.hp[ut];
                            res[nu] = 0;
                            ua[nu] = 0;
                            par[nu] = -1;
                            cell[ny * W + nx] = (uint16_t)nu;
                            if (po) snap[nu] = 0;  // produced this step: in no snapshot
                        }
                        nu++;
                        addPres(pl, -U.cost[ut]);
                        wsync();
                    }
                } else {
                    addErr(E_NEG_RES);
                }
            } break;
            default: break;
        }
    }
    // cycleLanes' lane-parallel MOVEs, after the movers' old cells are cleared and synced: lane = unit slot, `np` the
    // new cell (x, y are the low bytes of the core word: direction prm adds -256, 1, 256, -1 to them)
    DEV void moveBatch(bool mv, uint32_t cu, int prm, int np, bool check) {
        if (!mv) return;
        if (check && MRTS_UNLIKELY(cell[np] != EMPTY)) atomicOr(&hdr[H_ERR], (int32_t)E_COLLISION);
        cell[np] = (uint16_t)lid();
        const uint32_t step = (uint32_t)(0xFFFF01000001FF00ull >> (((uint32_t)prm & 3u) * 16u));
        uc[lid()] = (cu & ~0xFFFFu) | ((cu + step) & 0xFFFFu);
    }
    // GameState.cycle (rts/GameState.java:553-571): time++, snapshot the ready assignments
    // (ETA + issue time <= time) in insertion order, then remove + execute each in that order.
    DEV void cycle() {
        time++;
        if (!steady || nu > 64) ixValid = false;  // (steady: cycleLanes keeps the index, see carryIndex)
        if (MRTS_LIKELY(nu <= 64)) {
            cycleLanes();
            return;
        }
        // gather the ready list into LDS (slot order), count R
        int R = 0;
        for (int o0 = 0; o0 < nu; o0 += 64) {
            const int o = o0 + lid();
            bool ready = false;
            if (o < nu) {
                const uint32_t a = ua[o];
                ready = (a & UA_PRESENT) && etaSlot(o) + at[o] <= time;
            }
            const uint64_t m = ballot(ready);
            const int idx = R + lanes_below(m);
            if (ready && idx < 64) {
                rslot[idx] = (uint16_t)o;
                rseq[idx] = as[o];
            }
            if (ready) ua[o] |= UA_READY;
            R += __popcll(m);
        }
        wsync();
        if (R == 0) return;
        if (R <= 64) {
            // rank by insertion sequence: lane k holds ready item k
            const int k = lid();
            const int myseq = k < R ? rseq[k] : INF;
            const int myslot = k < R ? rslot[k] : 0;
            int rank = 0;
            for (int j = 0; j < R; j++) rank += rl(myseq, j) < myseq;
            wsync();
            if (k < R) rslot[rank] = (uint16_t)myslot;
            wsync();
            // lane r now holds ready item r (insertion order).  Every ready assignment leaves the
            // map (ua's PRESENT/READY) before any executes: no execute reads another unit's flags.
            // NONE executes as a no-op, so only the other types run, one by one, from registers —
            // a unit's core word changes under another's execute only by a kill (tracked in `killed`).
            const int os = k < R ? rslot[k] : 0;
            uint32_t a = 0, cu = 0;
            int prm = 0;
            if (k < R) {
                a = ua[os];
                cu = uc[os];
                prm = par[os];
                ua[os] = a & ~(UA_READY | UA_PRESENT);
            }
            wsync();
            uint64_t work = ballot(k < R && ua_type(a) != T_NONE);
            killedLanes = 0;
            readySlot = k < R ? os : -1;
            while (work) {
                const int r = __builtin_ctzll(work);
                work &= work - 1;
                uint32_t c = uniu(rl((int)cu, r));
                if ((killedLanes >> r) & 1ull) c |= UC_DEAD;
                execute(rl(os, r), c, uniu(rl((int)a, r)) & ~(UA_READY | UA_PRESENT), rl(prm, r));
            }
            readySlot = -1;
        } else {  // > 64 ready assignments: repeated minimum search
            while (true) {
                int best = INF;
                for (int o = lid(); o < nu; o += 64)
                    if (ua[o] & UA_READY) best = min(best, as[o]);
                best = wave_min(best);
                if (best == INF) break;
                int os = INF;
                for (int o = lid(); o < nu; o += 64)
                    if ((ua[o] & UA_READY) && as[o] == best) os = o;
                os = wave_min(os);
                if (lid() == 0) ua[os] &= ~(UA_READY | UA_PRESENT);
                wsync();
                execute(os);
            }
        }
    }
    // cycle() with every unit in one wave: lane = unit.  Each ready assignment leaves the map first
    // (in parallel); NONE executes as a no-op, so only the other ready assignments are ordered — by
    // insertion sequence (unique), ranked in registers — and executed one by one from registers.
    DEV void cycleLanes() {
        const int l = lid();
        bool ready = false;
        uint32_t a = 0, cu = 0;
        int prm = 0, sq = 0;
        if (l < nu) {
            a = ua[l];
            cu = uc[l];
            prm = par[l];
            sq = as[l];
            const int t0 = at[l];
            if (a & UA_PRESENT) ready = etaFlat(ua_type(a), prm, ua_ut(a), utyp(cu)) + t0 <= time;
        }
        AB_ON(AB_CYCLERANK, ablCycleRank(l, a, cu, prm, sq));
        if (ready) ua[l] = a & ~(UA_READY | UA_PRESENT);
        const bool wk0 = ready && ua_type(a) != T_NONE;
        const uint64_t work0 = ballot(wk0);
        // steady: the cycle's ready MOVEs execute in one lane-parallel pass (moveBatch below) unless an ATTACK is
        // ready too; each mover's lane clears its old cell here, ahead of the wsync the ready pass needs anyway
        bool mv = false;
        uint64_t movers = 0;
        if (steady) {
            const bool attack = ballot(wk0 && ua_type(a) == T_ATTACK) != 0;
            mv = wk0 && ua_type(a) == T_MOVE && !attack;
            movers = ballot(mv);
            if (mv) cell[uy(cu) * W + ux(cu)] = EMPTY;
        }
        const bool wk = wk0 && !mv;
        const uint64_t work = work0 & ~movers;
        // steady, the carried issue index (carryIndex): a MOVE / PRODUCE that leaves the map gives its position back
        // (buildIndex's position; the unit stands where the assignment found it until its own execute).  A present
        // MOVE / PRODUCE holds a direction 0..3 (issueSafe's legality test turned any other into NONE), so the
        // direction's cell offset is byte prm of -W, 1, W, -1 (W <= 127), read by one sign-extending extract
        const bool mpA = steady && (a & UA_PRESENT) && (ua_type(a) == T_MOVE || ua_type(a) == T_PRODUCE);
        const uint32_t dirOffs = ((uint32_t)(-W) & 0xFFu) | 1u << 8 | ((uint32_t)W & 0xFFu) << 16 | 0xFFu << 24;
        const int ipos = uy(cu) * W + ux(cu) + __builtin_amdgcn_sbfe((int)dirOffs, (uint32_t)prm * 8u, 8u) + W;
        if (steady) {
            if (mpA && ready) atomicAnd(&bits[ipos >> 5], ~(1u << (ipos & 31)));
            if (ballot(wk && ua_type(a) == T_PRODUCE)) prodDirty = true;
        }
        wsync();
        if (!work0) return;
        if (steady && movers) {
            // The ready MOVEs of a cycle without a ready ATTACK, all at once (UnitAction.execute's TYPE_MOVE,
            // rts/UnitAction.java:338-465, for each): the serial loop's order between them and the cycle's other
            // assignments changes nothing, because
            // * no mover is dead or dies here: only ATTACK and HARVEST kill (kill), no ATTACK is ready, and a HARVEST
            //   kills a resource unit, which holds no assignment;
            // * no two present MOVE / PRODUCE assignments share a target (the issue pass refuses the second;
            //   carryIndex's `bits` rests on the same fact), and a target was free when its assignment was issued and
            //   reserved since, while a mover stands on its old cell from before its MOVE was issued until now: no
            //   other MOVE or PRODUCE reads or writes a mover's old or new cell;
            // * HARVEST and RETURN act on the occupant of their target cell only if it is a resource / a stockpile,
            //   which no mover is: they find a mover or an empty cell there, before its move or after, and do nothing
            //   either way (the target's own resource or base gone earlier);
            // * the other executes touch res / hp / the players' resources / a new unit's slot, never a mover's words.
            // Old cells were cleared before the wsync above; E_COLLISION as the serial MOVE reports it.
            moveBatch(mv, cu, prm, ipos - W, true);
            AB_ON(AB_MOVEBATCH, ablMoveBatch(mv, cu, prm, ipos - W));
            wsync();
        }
        if (!work) return;
        int rank = 0;
        for (uint64_t m = work; m; m &= m - 1) rank += rl(sq, __builtin_ctzll(m)) < sq;
        killedLanes = 0;
        readySlot = wk ? l : -1;
        const int nw = __popcll(work);
        AB_ON(AB_EXECLOOP, ablExecLoop(wk, rank, nw, cu, a, prm));
        for (int r = 0; r < nw; r++) {
            const int k = __builtin_ctzll(ballot(wk && rank == r));
            uint32_t c = uniu((uint32_t)rl((int)cu, k));
            if ((killedLanes >> k) & 1ull) c |= UC_DEAD;
            execute(k, c, uniu((uint32_t)rl((int)a, k)) & ~(UA_READY | UA_PRESENT), rl(prm, k));
        }
        readySlot = -1;
        // steady: a unit killed in the loop takes its assignment with it (kill: GameState.removeUnit,
        // rts/GameState.java:79-82) — one still present was not ready, so its unit has not moved this cycle
        if (steady && deaths) {
            const bool gone = mpA && !ready && (uc[l] & UC_DEAD);
            if (gone) atomicAnd(&bits[ipos >> 5], ~(1u << (ipos & 31)));
            if (ballot(gone && ua_type(a) == T_PRODUCE)) prodDirty = true;
        }
    }
    // PhysicalGameState.gameover/winner (rts/PhysicalGameState.java:334-387)
    DEV void outcome(bool& gameover, int& winner) {
        int c0 = 0, c1 = 0;
        for (int o0 = 0; o0 < nu; o0 += 64) {
            const int o = o0 + lid();
            const uint32_t c = o < nu ? uc[o] : UC_DEAD;
            const bool live = !(c & UC_DEAD);
            c0 += __popcll(ballot(live && uplay(c) == 0));
            c1 += __popcll(ballot(live && uplay(c) == 1));
        }
        gameover = (c0 + c1 == 0) || ((c0 > 0) != (c1 > 0));
        winner = (c0 > 0 && c1 == 0) ? 0 : ((c1 > 0 && c0 == 0) ? 1 : -1);
    }
    // GameState.isComplete (rts/GameState.java:148-157): every owned unit has an assignment
    DEV bool complete() const {
        bool idle = false;
        for (int o0 = 0; o0 < nu; o0 += 64) {
            const int o = o0 + lid();
            if (o < nu) {
                const uint32_t c = uc[o];
                idle |= !(c & UC_DEAD) && uplay(c) >= 0 && !(ua[o] & UA_PRESENT);
            }
        }
        return ballot(idle) == 0;
    }
    // order-preserving removal of dead slots (LinkedList.remove, PhysicalGameState.java:208-210)
    DEV void compact() {
        int base = 0;
        for (int o0 = 0; o0 < nu; o0 += 64) {
            const int o = o0 + lid();
            const bool alive = o < nu && !(uc[o] & UC_DEAD);
            const uint64_t m = ballot(alive);
            const int idx = base + lanes_below(m);
            uint32_t c = 0, a = 0, sb = 0;
            int32_t t0 = 0, t1 = 0;
            int16_t h = 0, r = 0, pr = 0;
            if (alive) {
                if (po) sb = snap[o];
                c = uc[o];
                a = ua[o];
                t0 = at[o];
                t1 = as[o];
                h = hp[o];
                r = res[o];
                pr = par[o];
            }
            wsync();
            if (alive) {
                if (po) snap[idx] = (uint8_t)sb;
                uc[idx] = c;
                ua[idx] = a;
                at[idx] = t0;
                as[idx] = t1;
                hp[idx] = h;
                res[idx] = r;
                par[idx] = pr;
            }
            wsync();
            base += __popcll(m);
        }
        nu = base;
        for (int c = lid(); c < HW; c += 64)
            if (cell[c] != WALL) cell[c] = EMPTY;
        wsync();
        placeUnits();
    }

    // ------------------------------------------------------------------ reward functions
    // CloserToEnemyBaseRewardFunction.java:16-60 (and the identical CloserToEnemyUnit text): the enemy
    // Base is the first unit of minplayer named "Base" in the pre-cycle list; distances are from
    // maxplayer's Light/Heavy/Ranged/Worker units.  Squared distances are exact integers and sqrt is
    // monotone, so min(sqrt) = sqrt(min).
    DEV bool mobileType(int t) const { return (U.flags[t] & (N_WORKER | N_COMBAT)) != 0; }  // Light/Heavy/Ranged/Worker
    DEV void closerBefore() {
        int b0 = -1, b1 = -1;
        for (int o0 = 0; o0 < nu; o0 += 64) {
            const int o = o0 + lid();
            const uint32_t c = o < nu ? uc[o] : UC_DEAD;
            const bool base = !(c & UC_DEAD) && (U.flags[utyp(c)] & N_BASE);
            const uint64_t m0 = ballot(base && uplay(c) == 0), m1 = ballot(base && uplay(c) == 1);
            if (b0 < 0 && m0) b0 = o0 + __builtin_ctzll(m0);
            if (b1 < 0 && m1) b1 = o0 + __builtin_ctzll(m1);
        }
        hset(HX_BASE, b0 >= 0 ? (int)(uniu(uc[b0]) & 0xFFFFu) : -1);
        hset(HX_BASE + 1, b1 >= 0 ? (int)(uniu(uc[b1]) & 0xFFFFu) : -1);
        int o0, o1;
        closerMin(o0, o1);
        hset(HX_OLDSQ, o0);
        hset(HX_OLDSQ + 1, o1);
    }
    // smallest squared distance of player p's mobile units to the other player's base (INF if none)
    DEV void closerMin(int& sq0, int& sq1) {
        const int basePos0 = hget(HX_BASE), basePos1 = hget(HX_BASE + 1);
        int m0 = INF, m1 = INF;
        for (int o = lid(); o < nu; o += 64) {
            const uint32_t c = uc[o];
            if ((c & UC_DEAD) || !mobileType(utyp(c))) continue;
            const int pl = uplay(c);
            const int bp = pl == 0 ? basePos1 : basePos0;
            if (pl < 0 || bp < 0) continue;
            const int dx = (bp & 0xFF) - ux(c), dy = (bp >> 8) - uy(c), d = dx * dx + dy * dy;
            if (pl == 0) m0 = min(m0, d);
            else m1 = min(m1, d);
        }
        sq0 = wave_min(m0);
        sq1 = wave_min(m1);
    }
    static DEV double closerDist(int sq) { return sq == INF ? 2000000000.0 : __builtin_sqrt((double)sq); }
    // computeReward of every a_rfs entry for the game's external slots (slot0 + i is player pl(i)),
    // written to reward / done [slot][R]; returns done of a_rfs[0] (drives the auto-reset,
    // JNIGridnetVecClient.java:247,272).  WinLoss: WinLossRewardFunction.java:16-24; ResourceGather:
    // ResourceGatherRewardFunction.java:22-42; ProduceWorker / ProduceBuilding / ProduceCombatUnit:
    // ProduceWorkerRewardFunction.java:20-30 (the other two: the same lines of their files); Attack:
    // AttackRewardFunction.java:20-36 (a legal attack always targets a minplayer unit of the pre-cycle
    // pgs).  Constants are float 1.
    // it: this launch's iteration (the step's place in the Responses ring, KDyn.resp_reward); never the steady instance
    DEV bool writeRewards(int slot0, int nslots, int pl0, int pl1, bool gameover, int winner, int it = 0) {
        const int R = D.n_rewards;
        int newSq0 = INF, newSq1 = INF;
        if (MRTS_UNLIKELY(D.reward_need & RN_CLOSER)) closerMin(newSq0, newSq1);
        bool resLeft = false;
        if (D.reward_need & RN_RESOURCES)
            for (int o0 = 0; o0 < nu; o0 += 64) {
                const int o = o0 + lid();
                resLeft |= ballot(o < nu && !(uc[o] & UC_DEAD) && (U.flags[utyp(uc[o])] & N_RESOURCE) && res[o] > 0) != 0;
            }
        const int k0 = (int)(D.reward_kinds4 & 15u);
        // the Responses ring (mrts_set_step_responses): reward / done point at the call's ring and each
        // iteration writes its own step there (resp_stride = n_slots * n_rewards; 0 = the plain buffers)
        const size_t ro = (size_t)((uint32_t)it * (uint32_t)D.resp_stride);
        const bool done0 = k0 == RF_WINLOSS ? gameover : (k0 == RF_RESOURCE_GATHER ? !resLeft : false);
        const int L = lid();
        if (R == 1 && k0 == RF_WINLOSS) {  // WinLoss alone (the common case): a wave-uniform branch, no switch
            if (L < nslots) {
                const int p = L ? pl1 : pl0;
                if (D.reward) D.reward[ro + slot0 + L] = gameover ? (winner == p ? 1.0 : -1.0) : 0.0;
                if (D.done) D.done[ro + slot0 + L] = gameover ? 1 : 0;
            }
            return done0;
        }
        if (L < nslots * R && (D.reward || D.done)) {
            const int i = L / R, j = L - i * R;
            const int p = i ? pl1 : pl0;
            const int kind = (int)((D.reward_kinds4 >> (4 * j)) & 15u);
            double r = 0.0;
            bool d = false;
            switch (kind) {
                case RF_WINLOSS:
                    d = gameover;
                    r = gameover ? (winner == p ? 1.0 : -1.0) : 0.0;
                    break;
                case RF_RESOURCE_GATHER:
                    r = (double)(rwc[p * RC_N + RC_HARVEST] + rwc[p * RC_N + RC_RETURN]);
                    d = !resLeft;
                    break;
                case RF_PRODUCE_WORKER: r = (double)rwc[p * RC_N + RC_PROD_WORKER]; break;
                case RF_PRODUCE_BUILDING: r = (double)rwc[p * RC_N + RC_PROD_BUILDING]; break;
                case RF_PRODUCE_COMBAT_UNIT: r = (double)rwc[p * RC_N + RC_PROD_COMBAT]; break;
                case RF_ATTACK: r = (double)rwc[p * RC_N + RC_ATTACK]; break;
                case RF_CLOSER_TO_ENEMY_BASE:
                case RF_CLOSER_TO_ENEMY_UNIT:
                    if (hdr[HX_BASE + 1 - p] >= 0)
                        r = closerDist(hdr[HX_OLDSQ + p]) - closerDist(p == 0 ? newSq0 : newSq1);
                    break;
            }
            if (D.reward) D.reward[ro + (size_t)(slot0 + i) * R + j] = r;
            if (D.done) D.done[ro + (size_t)(slot0 + i) * R + j] = d ? 1 : 0;
        }
        return done0;
    }

    // ------------------------------------------------------------------ observation
    // GameState.getVectorObservation (rts/GameState.java:922-968): 6 planes [C][H][W] int32.
    // Lane = 4 consecutive cells -> one dwordx4 store per plane.
    DEV void obsCell(int c, int player, int v[6]) const {
        const int s = cell[c];
        v[0] = v[1] = v[2] = v[3] = v[4] = 0;
        v[5] = (s == WALL) ? 1 : 0;
        if (s < CAP) {
            const uint32_t cu = uc[s];
            const uint32_t a = ua[s];
            const int pl = uplay(cu);
            v[0] = hp[s];
            v[1] = res[s];
            v[2] = pl >= 0 ? ((pl + player) % 2) + 1 : 0;
            v[3] = utyp(cu) + 1;
            v[4] = (a & UA_PRESENT) ? ua_type(a) : 0;
        }
    }
    // 16x16 full observability with every value below 256 (KDyn.obs_img): the five dynamic planes are
    // rendered as bytes into LDS by one pass over the unit list (lane = unit slot; a live unit owns its
    // cell, the dead are off the cell map, as in the gather below), then each lane's 4 cells x 5 planes
    // come back as zero-extended byte loads (LDS pipe, no VALU) straight into the dwordx4 stores.  The
    // cell-map gather costs the VALU-issue-bound c3 kernel ~150 VALU instructions per game-step more.
    // `snap` is the image (ldsBytes reserves 5 HW bytes there; snapshots exist only in PO games).
    DEV void writeObsFullImg(int slot0, int nslots, int player0) {
        uint8_t* const img = snap;
        const int l = lid();
        uint32_t* const iw = (uint32_t*)img;
#pragma unroll
        for (int i = 0; i < 5; i++) iw[l + 64 * i] = 0u;  // 5 x 256 bytes
        wsync();
        for (int s = l; s < nu; s += 64) {
            const uint32_t cu = uc[s];
            if (!(cu & UC_DEAD)) {
                const int c = uy(cu) * W + ux(cu), pl = uplay(cu);
                const uint32_t a = ua[s];
                img[c] = (uint8_t)hp[s];
                img[HW + c] = (uint8_t)res[s];
                img[2 * HW + c] = (uint8_t)(pl >= 0 ? ((pl + player0) % 2) + 1 : 0);
                img[3 * HW + c] = (uint8_t)(utyp(cu) + 1);
                img[4 * HW + c] = (uint8_t)((a & UA_PRESENT) ? ua_type(a) : 0);
            }
        }
        wsync();
        const int c4 = 4 * l;
        int v[6][4];
#pragma unroll
        for (int q = 0; q < 5; q++)
#pragma unroll
            for (int j = 0; j < 4; j++) v[q][j] = img[q * HW + c4 + j];
        const int npl = firstIt ? 6 : 5;  // the static terrain plane: first write of a launch only
        if (firstIt)
#pragma unroll
            for (int j = 0; j < 4; j++) v[5][j] = cell[c4 + j] == WALL ? 1 : 0;
        else
#pragma unroll
            for (int j = 0; j < 4; j++) v[5][j] = 0;
        int32_t* o0 = D.obs + (size_t)slot0 * D.C * HW;
        const __amdgpu_buffer_rsrc_t rs = bufRsrc(o0, (uint32_t)(nslots * D.C * HW * 4));
#pragma unroll
        for (int i = 0; i < 2; i++) {
            if (i >= nslots) break;
#pragma unroll
            for (int q = 0; q < 6; q++) {
                if (q >= npl) break;
                int w[4];
#pragma unroll
                for (int j = 0; j < 4; j++)  // the other player's owners: 0, 1, 2 -> 0, 2, 1 (bits 2v.. of 0b011000)
                    w[j] = (i && q == 2) ? (int)__builtin_amdgcn_ubfe(24u, 2u * (uint32_t)v[q][j], 2u) : v[q][j];
                const uint32_t off = (uint32_t)((i * D.C + q) * HW + c4);
                st4sc1(rs, off * 4u, w[0], w[1], w[2], w[3]);
            }
        }
        if (MRTS_UNLIKELY(D_OFF(obs8) != nullptr)) {  // the uint8 transport (mrts_set_exchange_bytes): every plane
            if (!firstIt)
#pragma unroll
                for (int j = 0; j < 4; j++) v[5][j] = cell[c4 + j] == WALL ? 1 : 0;
            uint8_t* b0 = D.obs8 + (size_t)slot0 * D.C * HW;
            for (int i = 0; i < nslots; i++)
#pragma unroll
                for (int q = 0; q < 6; q++) {
                    uint32_t w = 0;
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const int x = (i && q == 2 && v[q][j]) ? 3 - v[q][j] : v[q][j];  // the other player's owners
                        w |= (uint32_t)x << (8 * j);
                    }
                    *(uint32_t*)(b0 + (size_t)(i * D.C + q) * HW + c4) = w;
                }
        }
        if (MRTS_UNLIKELY(D_OFF(obs16) != nullptr)) {  // the int16 transport copy (mrts_set_obs16): every plane
            if (!firstIt)
#pragma unroll
                for (int j = 0; j < 4; j++) v[5][j] = cell[c4 + j] == WALL ? 1 : 0;
            int16_t* h0 = D.obs16 + (size_t)slot0 * D.C * HW;
            for (int i = 0; i < nslots; i++)
#pragma unroll
                for (int q = 0; q < 6; q++) {
                    int4 w4 = make_int4(v[q][0], v[q][1], v[q][2], v[q][3]);
                    if (i && q == 2) {
                        w4.x = w4.x ? 3 - w4.x : 0;
                        w4.y = w4.y ? 3 - w4.y : 0;
                        w4.z = w4.z ? 3 - w4.z : 0;
                        w4.w = w4.w ? 3 - w4.w : 0;
                    }
                    *(uint2*)(h0 + (size_t)(i * D.C + q) * HW + c4) = pk16(w4);
                }
        }
    }
    DEV void writeObsFull(int slot0, int nslots, int player0) {
        if (HW == 256 && !po && D_ON(obs_img) && nslots <= 2) {
            writeObsFullImg(slot0, nslots, player0);
            return;
        }
        int32_t* o0 = D.obs + (size_t)slot0 * D.C * HW;
        if (HW <= 64) {
            // small maps (8x8: c2): lane = cell, one LDS round for the cell entry and one for its
            // occupant's fields, one dword store per plane (64 lanes = 256 contiguous bytes) — the
            // 4-cells-per-lane form below would leave 48 of the 64 lanes idle and quadruple each
            // active lane's dependent work
            const int c = lid();
            if (c < HW) {
                const int sc = cell[c];
                const int s = sc < CAP ? sc : 0;
                const uint32_t cu = uc[s], ca = ua[s];
                const int ch = hp[s], cr = res[s];
                const bool occ = sc < CAP;
                const int pl = uplay(cu);
                int v[6];
                v[0] = occ ? ch : 0;
                v[1] = occ ? cr : 0;
                v[2] = (occ && pl >= 0) ? ((pl + player0) % 2) + 1 : 0;
                v[3] = occ ? utyp(cu) + 1 : 0;
                v[4] = (occ && (ca & UA_PRESENT)) ? ua_type(ca) : 0;
                v[5] = sc == WALL ? 1 : 0;
                const __amdgpu_buffer_rsrc_t rs = bufRsrc(o0, (uint32_t)(nslots * D.C * HW * 4));
                const int npl = firstIt ? 6 : 5;  // the static terrain plane: first write of a launch only
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    if (i >= nslots) break;
#pragma unroll
                    for (int q = 0; q < 6; q++) {
                        if (q >= npl) break;
                        // the other player's view differs only in the owner plane
                        const int x = (i && q == 2 && v[2]) ? 3 - v[2] : v[q];
                        const uint32_t off = (uint32_t)((i * D.C + q) * HW + c);
                        __builtin_amdgcn_raw_buffer_store_b32(x, rs, (int)(off * 4u), 0, 16);
                    }
                }
                if (MRTS_UNLIKELY(D_OFF(obs16) != nullptr)) {  // the int16 transport copy (mrts_set_obs16)
                    int16_t* h0 = D.obs16 + (size_t)slot0 * D.C * HW;
                    for (int i = 0; i < nslots; i++)
#pragma unroll
                        for (int q = 0; q < 6; q++)
                            h0[(size_t)(i * D.C + q) * HW + c] = (int16_t)((i && q == 2 && v[2]) ? 3 - v[2] : v[q]);
                }
                if (MRTS_UNLIKELY(D_OFF(obs8) != nullptr)) {  // the uint8 transport (mrts_set_exchange_bytes)
                    uint8_t* b0 = D.obs8 + (size_t)slot0 * D.C * HW;
                    for (int i = 0; i < nslots; i++)
#pragma unroll
                        for (int q = 0; q < 6; q++)
                            b0[(size_t)(i * D.C + q) * HW + c] = (uint8_t)((i && q == 2 && v[2]) ? 3 - v[2] : v[q]);
                }
            }
        } else if ((HW & 3) == 0) {
            for (int c4 = 4 * lid(); c4 < HW; c4 += 256) {
                // obsCell for 4 cells without branches: the 4 cell entries, then the occupants' 4
                // fields each (an empty cell reads slot 0 and is masked), so the lane waits for two
                // LDS rounds instead of one pair per occupied cell
                int sc[4];
#pragma unroll
                for (int j = 0; j < 4; j++) sc[j] = cell[c4 + j];
                uint32_t cu[4], ca[4];
                int ch[4], cr[4];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int s = sc[j] < CAP ? sc[j] : 0;
                    cu[j] = uc[s];
                    ca[j] = ua[s];
                    ch[j] = hp[s];
                    cr[j] = res[s];
                }
                int v[4][6];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const bool occ = sc[j] < CAP;
                    const int pl = uplay(cu[j]);
                    v[j][0] = occ ? ch[j] : 0;
                    v[j][1] = occ ? cr[j] : 0;
                    v[j][2] = (occ && pl >= 0) ? ((pl + player0) % 2) + 1 : 0;
                    v[j][3] = occ ? utyp(cu[j]) + 1 : 0;
                    v[j][4] = (occ && (ca[j] & UA_PRESENT)) ? ua_type(ca[j]) : 0;
                    v[j][5] = sc[j] == WALL ? 1 : 0;
                }
                const __amdgpu_buffer_rsrc_t rs = bufRsrc(o0, (uint32_t)(nslots * D.C * HW * 4));
                // the terrain plane (5) is static: within a multi-step launch only its first write stores it
                const int npl = firstIt ? 6 : 5;
#pragma unroll
                for (int pl = 0; pl < 6; pl++) {
                    if (pl >= npl) break;
                    st4sc1(rs, (uint32_t)(pl * HW + c4) * 4u, v[0][pl], v[1][pl], v[2][pl], v[3][pl]);
                }
                if (MRTS_UNLIKELY(D_OFF(obs16) != nullptr)) {  // the int16 transport copy (mrts_set_obs16)
                    int16_t* h0 = D.obs16 + (size_t)slot0 * D.C * HW;
#pragma unroll
                    for (int pl = 0; pl < 6; pl++) {
                        int4 w = make_int4(v[0][pl], v[1][pl], v[2][pl], v[3][pl]);
                        *(uint2*)(h0 + (size_t)pl * HW + c4) = pk16(w);
                        if (nslots == 2) {
                            if (pl == 2) {
                                w.x = w.x ? 3 - w.x : 0;
                                w.y = w.y ? 3 - w.y : 0;
                                w.z = w.z ? 3 - w.z : 0;
                                w.w = w.w ? 3 - w.w : 0;
                            }
                            *(uint2*)(h0 + (size_t)(D.C + pl) * HW + c4) = pk16(w);
                        }
                    }
                }
                if (nslots == 2) {  // the other player's view differs only in the owner plane
#pragma unroll
                    for (int pl = 0; pl < 6; pl++) {
                        if (pl >= npl) break;
                        int4 w = make_int4(v[0][pl], v[1][pl], v[2][pl], v[3][pl]);
                        if (pl == 2) {
                            w.x = w.x ? 3 - w.x : 0;
                            w.y = w.y ? 3 - w.y : 0;
                            w.z = w.z ? 3 - w.z : 0;
                            w.w = w.w ? 3 - w.w : 0;
                        }
                        st4sc1(rs, (uint32_t)((D.C + pl) * HW + c4) * 4u, w.x, w.y, w.z, w.w);
                    }
                }
            }
        } else {
            for (int i = 0; i < nslots; i++) {
                int32_t* o = o0 + (size_t)i * D.C * HW;
                for (int c = lid(); c < HW; c += 64) {
                    int v[6];
                    obsCell(c, player0 + i, v);
#pragma unroll
                    for (int pl = 0; pl < 6; pl++) o[(size_t)pl * HW + c] = v[pl];
                    if (D_OFF(obs16)) {
                        int16_t* h = D.obs16 + (size_t)(slot0 + i) * D.C * HW;
#pragma unroll
                        for (int pl = 0; pl < 6; pl++) h[(size_t)pl * HW + c] = (int16_t)v[pl];
                    }
                }
            }
        }
    }
    // The compact observation record of this game (KDyn.rec_out, mrts_internal.h recWords): the live
    // units in list order, one word each — every field GameState.getVectorObservation reads
    // (rts/GameState.java:922-968: hp, resources, owner, type, the assignment's action type; the
    // terrain plane is the map's).  Both players' observations follow from it (the owner plane is
    // ((owner + p) % 2) + 1), so one record per game replaces 2 x 6 x HW observation values on the
    // wire of the exchange (k_render_records rebuilds them).  More live units than the record holds
    // set E_RECORD (the exchange then reports an error).
    // Partially observable (po): the record holds what PartiallyObservableGameState.getVectorObservation
    // reads for both views (rts/PartiallyObservableGameState.java:82-154, as writeObsPO renders it) — every
    // unit of either view's snapshot in list order with its live fields (a dead one stays until the
    // compaction) and the snapshot byte (membership and seen action per view); walls and sight disks
    // follow on the receiving side from the map and the unit-type table.
    DEV void writeRecord(int it) {
        const int RU = D.rec_units;
        uint32_t* r = D.rec_out + ((size_t)it * D.n_sp_games + g) * (size_t)recWords(RU, po);
        if (po) {
            int n = 0;
            bool bad = false;
            for (int s0 = 0; s0 < nu; s0 += 64) {
                const int s = s0 + lid();
                const bool in = s < nu;  // every LDS read of the lane in one round (no dependent second round)
                const uint32_t sb = in ? (uint32_t)snap[s] : 0u, cu = in ? uc[s] : 0u;
                const int h = in ? hp[s] : 0, rs = in ? res[s] : 0;
                const bool inv = (sb & 3u) != 0;
                const uint64_t m = ballot(inv);
                const int idx = n + lanes_below(m);
                if (inv && idx < RU) {
                    bad |= h < -128 || h > 127 || rs < 0 || rs > 255;
                    r[1 + 2 * idx] = (uint32_t)(uy(cu) * W + ux(cu)) | (((uint32_t)h & 0xFFu) << 16) | ((uint32_t)rs << 24);
                    r[2 + 2 * idx] = (uint32_t)(utyp(cu) + 1) | ((uint32_t)(uplay(cu) + 1) << 4) | ((sb & 0xFFu) << 8);
                }
                n += __popcll(m);
            }
            const bool over = n > RU || ballot(bad) != 0;
            if (lid() == 0) r[0] = (uint32_t)(n < RU ? n : RU) | (over ? 0x80000000u : 0u);
            if (over) addErr(E_RECORD);
            return;
        }
        int n = 0;
        for (int s0 = 0; s0 < nu; s0 += 64) {
            const int s = s0 + lid();
            const bool in = s < nu;  // every LDS read of the lane in one round (no dependent second round)
            const uint32_t cu = in ? uc[s] : UC_DEAD, a = in ? ua[s] : 0u;
            const uint32_t hr = in ? ((uint32_t)hp[s] & 0xFFu) | (((uint32_t)res[s] & 0xFFu) << 8) : 0u;
            const bool live = !(cu & UC_DEAD);
            const uint64_t m = ballot(live);
            const int idx = n + lanes_below(m);
            if (live && idx < RU) {
                const uint32_t act = (a & UA_PRESENT) ? (uint32_t)ua_type(a) : 0u;
                r[1 + idx] = (uint32_t)(uy(cu) * W + ux(cu)) | (hr << 8) | ((uint32_t)(utyp(cu) + 1) << 24) |
                             ((uint32_t)(uplay(cu) + 1) << 27) | (act << 29);
            }
            n += __popcll(m);
        }
        if (lid() == 0) r[0] = (uint32_t)(n < RU ? n : RU) | (n > RU ? 0x80000000u : 0u);
        if (n > RU) addErr(E_RECORD);
    }
    // helper-wave launch: the observation's cells for the helper wave to render (lane = cell, HW <= 64),
    // player 0's view: word 0 = hp | resources << 16, word 1 = owner | type << 4 | action << 8 | wall << 12
    DEV void packObs(uint32_t* buf, bool terrainToo) const {  // terrainToo: bit 13 of every cell's second word
        const int c = lid();
        if (c < HW) {
            const int sc = cell[c];
            const int s = sc < CAP ? sc : 0;
            const uint32_t cu = uc[s], ca = ua[s];
            const bool occ = sc < CAP;
            const int pl = uplay(cu);
            const uint32_t v0 = occ ? (uint32_t)(uint16_t)hp[s] : 0u, v1 = occ ? (uint32_t)(uint16_t)res[s] : 0u;
            const uint32_t v2 = (occ && pl >= 0) ? (uint32_t)(pl + 1) : 0u, v3 = occ ? (uint32_t)utyp(cu) + 1 : 0u;
            const uint32_t v4 = (occ && (ca & UA_PRESENT)) ? (uint32_t)ua_type(ca) : 0u, v5 = sc == WALL ? 1u : 0u;
            buf[2 * c] = v0 | (v1 << 16);
            buf[2 * c + 1] = v2 | (v3 << 4) | (v4 << 8) | (v5 << 12) | (terrainToo ? 1u << 13 : 0u);
        }
    }
    // PartiallyObservableGameState.getVectorObservation (rts/PartiallyObservableGameState.java:82-154):
    // the snapshot's units (live fields, possibly dead) in list order, last writer per cell; the
    // snapshot's assignments; walls; own / enemy sight disks of the snapshot units (calculateVisibility, :156-179).
    // delta: the buffer holds this game's view-p render of the previous observation write and the PO
    // record (poVis / poPend / lsnap) describes it.  A cell's planes 0-5 come from the last snapshot
    // unit on it (its current hp, resources, owner, type and snapshot assignment), planes 6-7 from
    // the sight rows; so the cells that can differ are: those of units whose membership in the view
    // or rendered fields changed (before and after — slots keep their index until the compaction),
    // those of rendered units that died last step (gone from the list: poPend), and the exact XOR
    // of old and new sight rows.  Only the 4-cell chunks holding them are rendered and stored.
    // The passes that the renderers share are defined here, once: the plane values and the row chunks
    // for all four (the general writeObsPO, writeObsPOFast, writeObsPOFast2, the helper's renderPOPacked),
    // the unit chunks for the first three, the item list and the chunk render for the game wave's two
    // fast forms.

    // cell c's 4-cell chunk into a chunk bitmap (32 chunks = 128 cells per word)
    DEV void poMarkCell(uint32_t* bits, int c) const { atomicOr(&bits[c >> 7], 1u << ((c >> 2) & 31)); }
    // The eight plane values of one cell in view v.  occ: a unit of the view's snapshot is the cell's
    // last writer, with unit word cu, snapshot byte sb, hp h and resources r (ignored without one);
    // mr / tr: the words of the view's own / the other player's sight rows whose bit x is this cell's.
    DEV void poPlanes(int* o, bool occ, uint32_t cu, uint32_t sb, int h, int r, bool wall, int v, uint32_t mr, uint32_t tr, int x) const {
        const int pl = uplay(cu), sa = snap_act(sb, v);
        o[0] = occ ? h : 0;
        o[1] = occ ? r : 0;
        o[2] = (occ && pl >= 0) ? ((pl + v) % 2) + 1 : 0;
        o[3] = occ ? utyp(cu) + 1 : 0;
        o[4] = (occ && sa) ? sa - 1 : 0;
        o[5] = wall ? 1 : 0;
        o[6] = (int)((mr >> x) & 1u);
        o[7] = (int)((tr >> x) & 1u);
    }
    // A sight row's changed columns d (old XOR new row word: W <= 32) into the dirty bits of that
    // row's chunks.  k0 = the row's first chunk (W / 4 chunks per row, <= 8); the row's chunk bits
    // go out in one atomic unless they straddle two dirty words (24x24: k0 = 30 at y = 5).
    DEV void poRowChunks(uint32_t* dirty, uint32_t d, int k0) const {
        if (!d) return;
        uint32_t gbits = 0;  // bit j = column group 4j..4j+3 changed
#pragma unroll
        for (int j = 0; j < 8; j++) gbits |= ((d >> (4 * j)) & 0xFu) ? (1u << j) : 0u;
        if ((k0 & 31) + (W >> 2) <= 32) {
            atomicOr(&dirty[k0 >> 5], gbits << (k0 & 31));
        } else {
            for (uint32_t gg = gbits; gg; gg &= gg - 1) {
                const int k = k0 + __builtin_ctz(gg);
                atomicOr(&dirty[k >> 5], 1u << (k & 31));
            }
        }
    }
    // View v's change test for the unit of one slot, into the view's dirty bits.  in: the unit is in
    // the view now, at cell cc with snapshot byte sb and key = hp | resources << 16; had: the slot
    // held a unit at the previous render, at cell cp with that render's snapshot byte lsnapP and key
    // lkeyP.  A unit that entered or left the view, moved, or changed a rendered field dirties the
    // chunk it was rendered in and the chunk it is rendered in.
    DEV void poUnitChunks(uint32_t* dirty, int v, bool in, bool had, int cc, int cp, uint32_t sb, uint32_t key,
                          uint32_t lsnapP, uint32_t lkeyP) const {
        const bool inP = had && ((lsnapP >> v) & 1u);
        bool chg = in != inP;
        if (in && inP) chg = cc != cp || key != lkeyP || snap_act(sb, v) != (int)((lsnapP >> (2 + 3 * v)) & 7u);
        if (chg && inP) poMarkCell(dirty, cp);
        if (chg && in) poMarkCell(dirty, cc);
    }
    // A dirty bitmap into the item list: tag | k for every chunk k < HW / 4 whose bit is set (all:
    // for every chunk), in chunk order, from poList[n] on; the new item count.  Lane l of the whole
    // wave (ballots).  writeObsPOFast passes constants for `all` and `tag`, which fold away.
    DEV int poListChunks(int l, int n, const uint32_t* dirty, bool all, uint32_t tag) {
        const int NC = HW >> 2;
#pragma unroll
        for (int c0 = 0; c0 < 256; c0 += 64) {  // NC <= 256 (H, W <= 32)
            if (c0 < NC) {
                const int k = c0 + l;
                const bool dk = k < NC && (all || ((dirty[k >> 5] >> (k & 31)) & 1u));
                const uint64_t m = ballot(dk);
                if (dk) poList[n + lanes_below(m)] = (uint16_t)(tag | (uint32_t)k);
                n += __popcll(m);
            }
        }
        return n;
    }
    // Chunk c4's four cells in view v, as plane values o[cell][plane].  A cell's last snapshot writer
    // (list order) is the later of its live occupant, when that unit is in the view, and the view's
    // dead units on it (few), so no per-cell scratch map is built.  deadAll: the slots of the dead
    // units the wave walks (uniform: of both views in a two-view render); deadView: those of view v.
    // rows: the view's sight rows [mine H][theirs H].  Shared by the game wave's renders (writeObsPOFast,
    // writeObsPOFast2), which read the live LDS state; the helper wave's renderPOPacked reads a pack and
    // has the same loop over it.
    DEV void poChunk(int v, int c4, uint64_t deadAll, uint64_t deadView, const uint32_t* rows, int (&o)[4][8]) const {
        const int y = (4 * c4) / W, x0 = (4 * c4) % W;  // lane = 4 consecutive cells of one row
        int cs[4], sl[4];
#pragma unroll
        for (int j = 0; j < 4; j++) cs[j] = cell[4 * c4 + j];
        const uint32_t mr = rows[y], tr = rows[H + y];
        uint32_t ocu[4], osb[4];
        int ohp[4], ors[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {  // the live occupant's fields (an empty cell reads slot 0, masked)
            const int s = cs[j] < CAP ? cs[j] : 0;
            ocu[j] = uc[s];
            osb[j] = snap[s];
            ohp[j] = hp[s];
            ors[j] = res[s];
        }
#pragma unroll
        for (int j = 0; j < 4; j++) sl[j] = (cs[j] < CAP && snap_in(osb[j], v)) ? cs[j] : -1;
        for (uint64_t m = deadAll; m; m &= m - 1) {  // the view's dead units: a later list position wins
            const int ds = __builtin_ctzll(m);
            // the dead unit's fields from LDS, never by readlane: this loop is divergent (lanes >= n
            // are off), and the compiler may recompute a lane's cu / hp / snapshot byte inside it for
            // the active lanes only, so a readlane of an inactive lane returns a stale register
            // (round 4's soak saw the stale value in c5, round 5 found this cause in all three fast
            // renders: DESIGN.md §4)
            const uint32_t dcu = uc[ds];
            const int dcell = uy(dcu) * W + ux(dcu);
            const int dh = hp[ds], dr = res[ds];
            const uint32_t dsb = snap[ds];
            const bool mine = (deadView >> ds) & 1ull;
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (mine && dcell == 4 * c4 + j && ds > sl[j]) {
                    sl[j] = ds;
                    ocu[j] = dcu;
                    osb[j] = dsb;
                    ohp[j] = dh;
                    ors[j] = dr;
                }
        }
#pragma unroll
        for (int j = 0; j < 4; j++) poPlanes(o[j], sl[j] >= 0, ocu[j], osb[j], ohp[j], ors[j], cs[j] == WALL, v, mr, tr, x0 + j);
    }
    // writeObsPO for maps with W % 4 == 0, W <= 32 (one word per sight row), H <= 32, sight <= 15
    // and every unit in one wave (lane = slot).  One unit pass paints the sight disks, marks the
    // chunks of changed units (delta) and of the view's dead units (the next record's pending
    // chunks).  Same output as the general form below.
    DEV void writeObsPOFast(int slot, int p, bool delta) {
        const int l = lid(), NCW = poChunkWords(HW), NC = HW >> 2;
        uint32_t* dirty = poDirty;
        uint32_t* nextPend = poDirty + NCW;
        int32_t* pr = D.po_prev ? D.po_prev + (size_t)g * D.po_words : nullptr;
        const int SW = poSnapWords(CAP);
        const int nu0 = delta ? hget(H_NU) : 0;  // the header holds the loaded unit count until store()
        if (l < 2 * H) vis[l] = 0;  // [mine H][theirs H]
        if (l < NCW) {
            dirty[l] = delta ? poPend[p * NCW + l] : 0u;
            nextPend[l] = 0u;
        }
        const bool live = l < nu;
        uint32_t cu = 0, sb = 0;
        int hv = 0, rv = 0;
        if (live) {
            cu = uc[l];
            sb = snap[l];
            hv = hp[l];
            rv = res[l];
        }
        const bool in = live && snap_in(sb, p);
        const bool dead = in && (cu & UC_DEAD);
        const int cc = uy(cu) * W + ux(cu);
        wsync();
        // visibility planes over the view's units at their current positions (dead ones included:
        // the view's list still holds them): own / other player's sight disks
        const bool painter = in && uplay(cu) >= 0;
        AB_SKIP(AB_PO_NOPAINT)
        if (ballot(painter)) paintDisks(painter, cu, uplay(cu) == p ? vis : vis + H);
        const uint64_t deadM = ballot(dead);
        if (pr && dead) poMarkCell(nextPend, cc);
        if (delta && (live || l < nu0)) {
            const uint32_t key = (uint32_t)(uint16_t)hv | ((uint32_t)(uint16_t)rv << 16);
            poUnitChunks(dirty, p, in, l < nu0, cc, uy(lcu) * W + ux(lcu), sb, key, lsnap, lkey);
        }
        wsync();
        if (l < 2 * H) {  // sight rows: changed columns -> chunk bits of that row; the record's copy
            const uint32_t row = vis[l];
            if (delta) poRowChunks(dirty, row ^ poVis[p * 2 * H + l], (l < H ? l : l - H) * (W >> 2));
            if (pr) pr[1 + SW + p * 2 * H + l] = (int32_t)row;
        }
        wsync();
        const int n = delta ? poListChunks(l, 0, dirty, false, 0u) : NC;  // chunks to render: the dirty list, or all
        if (pr && l < NCW) pr[1 + SW + 4 * H + p * NCW + l] = (int32_t)nextPend[l];
        wsync();
        int32_t* out = D.obs + (size_t)slot * D.C * HW;
        for (int it = l; it < n; it += 64) {
            const int c4 = delta ? (int)poList[it] : it;
            int v[4][8];
            poChunk(p, c4, deadM, deadM, vis, v);
            const __amdgpu_buffer_rsrc_t rs = bufRsrc(out, (uint32_t)(D.C * HW * 4));
#pragma unroll
            for (int k = 0; k < 8; k++) st4sc1(rs, (uint32_t)(k * HW + 4 * c4) * 4u, v[0][k], v[1][k], v[2][k], v[3][k]);
        }
        wsync();
    }
    // writeObsPOFast for both views of a self-play game in one pass (slot0 + v renders player v's
    // view v): the unit pass reads each unit once and paints its disk into both views' rows, the
    // dirty chunks of both views go into one list, and each render lane takes one (view, chunk)
    // item — half the dependent LDS rounds of two writeObsPOFast calls.  delta: bit v = view v's
    // buffer holds its previous render (writeObsPOFast's delta).  Same output as
    // writeObsPOFast(slot0, 0, delta & 1) followed by writeObsPOFast(slot0 + 1, 1, delta >> 1 & 1).
    // The record's global copy is for the next launch: inside a multi-step launch this render keeps the
    // record in LDS (poLds: poVis, poPend) and the next iteration reads it there, so only the last
    // iteration stores it (the sight rows and pending chunks here, the snapshot bytes in poRecordSnaps).
    DEV void writeObsPOFast2(int slot0, uint32_t delta) {
        const int l = lid();
        uint32_t* const rowsV0 = vis;  // [mine H][theirs H]
        const int nu0 = delta ? hget(H_NU) : 0;  // the header holds the loaded unit count until store()
        const int NCW = poChunkWords(HW);
        uint32_t* const rowsV1 = vis2;
        int32_t* pr = D.po_prev ? D.po_prev + (size_t)g * D.po_words : nullptr;
        int32_t* const prG = (!iter || lastIt) ? pr : nullptr;
        const int SW = poSnapWords(CAP);
        const bool d0 = delta & 1u, d1 = (delta >> 1) & 1u;
        if (l < 2 * H) {
            rowsV0[l] = 0;
            rowsV1[l] = 0;
        }
        if (l < NCW) {  // [view][dirty, next pending]
            poDirty[l] = d0 ? poPend[l] : 0u;
            poDirty[NCW + l] = 0u;
            poDirty[2 * NCW + l] = d1 ? poPend[NCW + l] : 0u;
            poDirty[3 * NCW + l] = 0u;
        }
        const bool live = l < nu;
        uint32_t cu = 0, sb = 0;
        int hv = 0, rv = 0;
        if (live) {
            cu = uc[l];
            sb = snap[l];
            hv = hp[l];
            rv = res[l];
        }
        const bool in0 = live && snap_in(sb, 0), in1 = live && snap_in(sb, 1);
        const bool isDead = (cu & UC_DEAD) != 0;
        const bool dead0 = in0 && isDead, dead1 = in1 && isDead;
        const int cc = uy(cu) * W + ux(cu);
        const int own = uplay(cu);
        wsync();
        {
            const bool pt0 = in0 && own >= 0, pt1 = in1 && own >= 0;
            AB_SKIP(AB_PO_NOPAINT)
            if (ballot(pt0 || pt1))
                paintDisks2(pt0, own == 0 ? rowsV0 : rowsV0 + H, pt1, own == 1 ? rowsV1 : rowsV1 + H, cu);
        }
        const uint64_t deadM0 = ballot(dead0), deadM1 = ballot(dead1);
        if (pr && dead0) poMarkCell(poDirty + NCW, cc);
        if (pr && dead1) poMarkCell(poDirty + 3 * NCW, cc);
        if (delta && (live || l < nu0)) {
            const int cp = uy(lcu) * W + ux(lcu);
            const uint32_t key = (uint32_t)(uint16_t)hv | ((uint32_t)(uint16_t)rv << 16);
            if (d0) poUnitChunks(poDirty, 0, in0, l < nu0, cc, cp, sb, key, lsnap, lkey);
            if (d1) poUnitChunks(poDirty + 2 * NCW, 1, in1, l < nu0, cc, cp, sb, key, lsnap, lkey);
        }
        wsync();
        if (l < 2 * H) {  // sight rows: changed columns -> chunk bits of that row; the record's copies
            const int k0 = (l < H ? l : l - H) * (W >> 2);
#pragma unroll
            for (int v = 0; v < 2; v++) {
                const uint32_t row = (v ? rowsV1 : rowsV0)[l];
                if (v ? d1 : d0) poRowChunks(poDirty + 2 * v * NCW, row ^ poVis[v * 2 * H + l], k0);
                // the record's LDS copy.  Only this lane reads or writes this word of poVis between the
                // barriers around this pass, so the store may sit anywhere after the read above.
                poVis[v * 2 * H + l] = row;
                if (prG) prG[1 + SW + v * 2 * H + l] = (int32_t)row;
            }
        }
        wsync();
        // one list of (view << 15 | chunk) items: view 0's dirty chunks (all, without delta), then view 1's
        int n = poListChunks(l, 0, poDirty, !d0, 0u);
        n = poListChunks(l, n, poDirty + 2 * NCW, !d1, 1u << 15);
        if (pr && l < NCW) {
            if (prG) {
                prG[1 + SW + 4 * H + l] = (int32_t)poDirty[NCW + l];
                prG[1 + SW + 4 * H + NCW + l] = (int32_t)poDirty[3 * NCW + l];
            }
            poPend[l] = poDirty[NCW + l];  // LDS copies, as the sight rows above
            poPend[NCW + l] = poDirty[3 * NCW + l];
        }
        poLds = pr != nullptr;
        wsync();
        AB_ON(AB_COUNT, ablCountRender(l, n, delta));
        AB_ON(AB_PO_NOSTORE, n = 0);  // no render pass (gather + stores)
        int32_t* out = D.obs + (size_t)slot0 * D.C * HW;
        const __amdgpu_buffer_rsrc_t rs = bufRsrc(out, (uint32_t)(2 * D.C * HW * 4));
        const uint64_t deadAny = deadM0 | deadM1;
        for (int it = l; it < n; it += 64) {
            const uint32_t e = poList[it];
            const int v = (int)(e >> 15), c4 = (int)(e & 0x7FFFu);
            int vv[4][8];
            poChunk(v, c4, deadAny, v ? deadM1 : deadM0, v ? rowsV1 : rowsV0, vv);
            const uint32_t base = (uint32_t)(v * D.C * HW + 4 * c4) * 4u;
            AB_ON(AB_PO_ZEROSTORE, ablKeepChunk(vv));  // pricing: the render's values computed (kept alive), not stored
            AB_SKIP(AB_PO_ZEROSTORE)
#pragma unroll
            for (int k = 0; k < 8; k++) st4sc1(rs, base + (uint32_t)(k * HW) * 4u, vv[0][k], vv[1][k], vv[2][k], vv[3][k]);
        }
        wsync();
    }
    DEV bool poFast2() const { return (W & 3) == 0 && W <= 32 && H <= 32 && nu <= 64 && U.maxSight <= 15; }
    // the helper's part of a packed step's masks (writeMasksLanes with recOut): each own idle unit's
    // mask record (79 bytes from its 3 bit words) and fused-policy row, and the zero record + zero row
    // of every vacated cell — the same bytes the game wave would have stored.  Lane l = threadIdx.x - 64.
    DEV void storeRecordsHelp(const uint32_t* rb) {
        const int l = (int)threadIdx.x - 64;
        const int total = HW * K, slot0 = 2 * g;
        uint8_t* const masks = D.masks;  // read ahead of the early return: where this load sits is part of the measured code
        if (!(uniu(rb[5 * 64]) >> 31)) return;  // the game wave stored this step's masks itself
        const uint32_t e = rb[l];
        if (e != ~0u) {
            const int si = (int)(e >> 16), c = (int)(e & 0xFFFFu), slot = slot0 + si;
            const uint64_t lo = (uint64_t)rb[64 + l] | ((uint64_t)rb[128 + l] << 32);
            const uint32_t w2 = rb[192 + l];
            storeRecord(masks + (size_t)slot * total + (size_t)c * K, lo, w2);
            if (D_HAS(pol_actions) && D_ON(pol_delta)) {
                int32_t a[7];
                unpackFwd(rb[256 + l], a);
                int32_t* dst = D.pol_actions + ((size_t)slot * HW + c) * 7;
                st4u<WT_MASK>(dst, a[0], a[1], a[2], a[3]);
                st3u<WT_MASK>(dst + 4, a[4], a[5], a[6]);
            }
        }
        const int ngone = (int)(uniu(rb[5 * 64]) & 0xFFFFu);
        const uint16_t* gl = (const uint16_t*)(rb + 5 * 64 + 1);
        if (l < ngone) {
            const uint32_t ge = gl[l];
            const int slot = slot0 + (int)(ge >> 15), cz = (int)(ge & 0x7FFFu);
            storeRecord(masks + (size_t)slot * total + (size_t)cz * K, 0ull, 0u);
            if (D_HAS(pol_actions) && D_ON(pol_delta)) {
                int32_t* dst = D.pol_actions + ((size_t)slot * HW + cz) * 7;
                st4u<WT_MASK>(dst, 0, 0, 0, 0);
                st3u<WT_MASK>(dst + 4, 0, 0, 0);
            }
        }
    }
    // Helper-wave launch, partially observable self-play (k_env HELP && FPO, BASELINE c5): the game
    // wave hands this step's render inputs to the helper wave instead of rendering (writeObsPOFast2's
    // unit pass reads, per unit slot < 64: the unit word, hp | resources, the snapshot byte, and the
    // previous record's position / key / snapshot byte; the assignment type + 1 for the next step's
    // snapshot, snapFromPack), and the helper renders while the game runs its compaction, masks,
    // policy and the next step.  pk = [5][64] words, ph = [4] header words:
    // unit count, the previous record's unit count, flags (bits 0-1 delta per view, `how`: bit 2 =
    // render the pack, bit 3 = render the live state with writeObsPO, the game waiting).
    DEV void packPO(uint32_t* pk, uint32_t* ph, uint32_t delta, uint32_t how) {
        const int l = lid();
        const bool live = l < nu;
        pk[l] = live ? uc[l] : 0u;
        pk[64 + l] = live ? ((uint32_t)(uint16_t)hp[l] | ((uint32_t)(uint16_t)res[l] << 16)) : 0u;
        const uint32_t a = live ? ua[l] : 0u;
        pk[128 + l] = (live ? (uint32_t)snap[l] : 0u) | ((lsnap & 0xFFu) << 8) |
                      ((a & UA_PRESENT) ? (uint32_t)(ua_type(a) + 1) << 16 : 0u);
        pk[192 + l] = lcu;
        pk[256 + l] = lkey;
        if (l == 0) {
            ph[0] = (uint32_t)nu;
            ph[1] = (uint32_t)hget(H_NU);
            ph[2] = (delta & 3u) | how;
        }
        // how = 4: the helper keeps the record's LDS copies, as writeObsPOFast2 does; 8: the general
        // render stores it globally only, and nextStep re-reads it
        poLds = how == 4u && D.po_prev != nullptr;
    }
    // snapshotBoth of the NEXT step, by the helper wave from step k's pack: the state the next step
    // starts from is the packed one after the end-of-step compaction (dead units leave, the rest keep
    // their order and positions, assignments and liveness do not change in between), so each live
    // unit paints its sight disk into its player's rows and takes the membership bits and view 0's
    // assignment bits at its compacted index.  hsnap[slot] = the snapshot byte.
    DEV void snapFromPack(const uint32_t* pk, const uint32_t* ph, uint32_t* rows, uint8_t* hsnap) {
        const int l = (int)threadIdx.x - 64;
        const int nuP = (int)uniu(ph[0]);
        uint32_t* const r0 = rows;
        uint32_t* const r1 = rows + H;
        if (l < 2 * H) rows[l] = 0;
        const uint32_t cu = l < nuP ? pk[l] : UC_DEAD;
        const bool live = !(cu & UC_DEAD);
        const int own = uplay(cu);
        const uint32_t at = (pk[128 + l] >> 16) & 15u;  // assignment type + 1 (0 = none)
        wsync();
        paintDisks2(live && own == 0, r0, live && own == 1, r1, cu);
        wsync();
        const uint64_t m = ballot(live);
        if (live) {
            const int x = ux(cu), y = uy(cu);
            const bool in0 = (r0[y] >> x) & 1u, in1 = (r1[y] >> x) & 1u;
            hsnap[lanes_below(m)] = (uint8_t)((in0 ? 1u : 0u) | (in1 ? 2u : 0u) | (in0 ? at << 2 : 0u));
        }
        wsync();
    }
    // the game wave's side: the helper's snapshot bytes instead of snapshotBoth (same bytes, same header)
    DEV void takeSnap(const uint8_t* hsnap) {
        const int l = lid();
        if (l < nu) snap[l] = hsnap[l];
        hset(HX_SNAP + 0, seq);
        wsync();
    }
    // writeObsPOFast2 as run by the helper wave (lane l = threadIdx.x - 64) from a packed step (packPO):
    // the same passes and stores, written out here and not shared with it beyond poPlanes and
    // poRowChunks: built from the game wave's shared passes over a pack-reading source, the c5 helper
    // instance measured 0.4 - 1.2 % slower (profiles/po_render_refactor.md).  What the game wave's live LDS state gave it comes from the pack:
    // the units' fields, and the live occupant of a cell from hcell (slot, or 0xFF), a per-step map
    // built here from the packed positions (a unit in the list and not dead = the game's cell map);
    // walls from the game's cell map (WALL entries are static: units never stand on walls).  rowsV0 =
    // the helper's own view-0 sight rows (the game wave's snapshots use `vis` meanwhile).  last: the
    // launch's last iteration stores the record's sight rows and pending chunks globally.
    DEV void renderPOPacked(const uint32_t* pk, const uint32_t* ph, uint32_t* rowsV0, uint8_t* hcell, bool last) {
        const int l = (int)threadIdx.x - 64;
        const int NCW = poChunkWords(HW), NC = HW >> 2;
        uint32_t* const rowsV1 = vis2;
        int32_t* pr = D.po_prev ? D.po_prev + (size_t)g * D.po_words : nullptr;
        int32_t* const prG = last ? pr : nullptr;
        const int SW = poSnapWords(CAP);
        const int nuP = (int)ph[0], nu0 = (int)ph[1];
        const uint32_t delta = ph[2] & 3u;
        const bool d0 = delta & 1u, d1 = (delta >> 1) & 1u;
        if (l < 2 * H) {
            rowsV0[l] = 0;
            rowsV1[l] = 0;
        }
        if (l < NCW) {
            poDirty[l] = d0 ? poPend[l] : 0u;
            poDirty[NCW + l] = 0u;
            poDirty[2 * NCW + l] = d1 ? poPend[NCW + l] : 0u;
            poDirty[3 * NCW + l] = 0u;
        }
        for (int i = l; i < HW / 8; i += 64) ((uint2*)hcell)[i] = make_uint2(~0u, ~0u);  // (8-byte aligned)
        const bool live = l < nuP;
        const uint32_t cu = pk[l], kv = pk[64 + l], sw = pk[128 + l];
        const uint32_t lcuP = pk[192 + l], lkeyP = pk[256 + l];
        const uint32_t sb = sw & 0xFFu, lsnapP = (sw >> 8) & 0xFFu;
        const int hv = (int)(int16_t)(kv & 0xFFFFu), rv = (int)(int16_t)(kv >> 16);
        const bool in0 = live && snap_in(sb, 0), in1 = live && snap_in(sb, 1);
        const bool isDead = (cu & UC_DEAD) != 0;
        const bool dead0 = in0 && isDead, dead1 = in1 && isDead;
        const int cc = uy(cu) * W + ux(cu);
        const int own = uplay(cu);
        wsync();
        if (live && !isDead) hcell[cc] = (uint8_t)l;
        {
            const bool pt0 = in0 && own >= 0, pt1 = in1 && own >= 0;
            if (ballot(pt0 || pt1))
                paintDisks2(pt0, own == 0 ? rowsV0 : rowsV0 + H, pt1, own == 1 ? rowsV1 : rowsV1 + H, cu);
        }
        const uint64_t deadM0 = ballot(dead0), deadM1 = ballot(dead1);
        if (pr && dead0) atomicOr(&poDirty[NCW + (cc >> 7)], 1u << ((cc >> 2) & 31));
        if (pr && dead1) atomicOr(&poDirty[3 * NCW + (cc >> 7)], 1u << ((cc >> 2) & 31));
        if (delta && (live || l < nu0)) {
            const int cp = uy(lcuP) * W + ux(lcuP);
            const uint32_t key = (uint32_t)(uint16_t)hv | ((uint32_t)(uint16_t)rv << 16);
#pragma unroll
            for (int v = 0; v < 2; v++) {
                if (!(v ? d1 : d0)) continue;
                const bool in = v ? in1 : in0;
                const bool inP = l < nu0 && ((lsnapP >> v) & 1u);
                bool chg = in != inP;
                if (in && inP)
                    chg = cc != cp || key != lkeyP || snap_act(sb, v) != (int)((lsnapP >> (2 + 3 * v)) & 7u);
                uint32_t* dirty = poDirty + 2 * v * NCW;
                if (chg && inP) atomicOr(&dirty[cp >> 7], 1u << ((cp >> 2) & 31));
                if (chg && in) atomicOr(&dirty[cc >> 7], 1u << ((cc >> 2) & 31));
            }
        }
        wsync();
        if (l < 2 * H) {  // sight rows: changed columns -> chunk bits of that row; the record's copies
            const int y = l < H ? l : l - H;
            const int k0 = y * (W >> 2);
#pragma unroll
            for (int v = 0; v < 2; v++) {
                const uint32_t row = (v ? rowsV1 : rowsV0)[l];
                if (v ? d1 : d0) {
                    const uint32_t d = row ^ poVis[v * 2 * H + l];
                    poRowChunks(poDirty + 2 * v * NCW, d, k0);
                }
                poVis[v * 2 * H + l] = row;  // the record's LDS copy (the next render)
                if (prG) prG[1 + SW + v * 2 * H + l] = (int32_t)row;
            }
        }
        wsync();
        int n = 0;  // (view << 15 | chunk) items: view 0's dirty chunks (all, without delta), then view 1's
#pragma unroll
        for (int v = 0; v < 2; v++) {
            const bool dv = v ? d1 : d0;
            const uint32_t* dirty = poDirty + 2 * v * NCW;
#pragma unroll
            for (int c0 = 0; c0 < 256; c0 += 64) {  // NC <= 256 (H, W <= 32)
                if (c0 < NC) {
                    const int k = c0 + l;
                    const bool dk = k < NC && (!dv || ((dirty[k >> 5] >> (k & 31)) & 1u));
                    const uint64_t m = ballot(dk);
                    if (dk) poList[n + lanes_below(m)] = (uint16_t)((v << 15) | k);
                    n += __popcll(m);
                }
            }
        }
        if (pr && l < NCW) {
            if (prG) {
                prG[1 + SW + 4 * H + l] = (int32_t)poDirty[NCW + l];
                prG[1 + SW + 4 * H + NCW + l] = (int32_t)poDirty[3 * NCW + l];
            }
            poPend[l] = poDirty[NCW + l];
            poPend[NCW + l] = poDirty[3 * NCW + l];
        }
        wsync();
        int32_t* out = D.obs + (size_t)(2 * g) * D.C * HW;
        const __amdgpu_buffer_rsrc_t rs = bufRsrc(out, (uint32_t)(2 * D.C * HW * 4));
        const uint64_t deadAny = deadM0 | deadM1;
        for (int it = l; it < n; it += 64) {
            const uint32_t e = poList[it];
            const int v = (int)(e >> 15), c4 = (int)(e & 0x7FFFu);  // lane = 4 consecutive cells of one row
            const uint64_t deadM = v ? deadM1 : deadM0;
            const int y = (4 * c4) / W, x0 = (4 * c4) % W;
            const uint32_t* rows = v ? rowsV1 : rowsV0;
            const uint32_t occ4 = ((const uint32_t*)hcell)[c4];
            int cs[4], sl[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t o = (occ4 >> (8 * j)) & 0xFFu;
                cs[j] = o != 0xFFu ? (int)o : (cell[4 * c4 + j] == WALL ? (int)WALL : (int)EMPTY);
            }
            const uint32_t mr = rows[y], tr = rows[H + y];
            uint32_t ocu[4], osb[4];
            int ohp[4], ors[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {  // the live occupant's fields (an empty cell reads slot 0, masked)
                const int s = cs[j] < CAP ? cs[j] : 0;
                ocu[j] = pk[s];
                const uint32_t k2 = pk[64 + s];
                osb[j] = pk[128 + s] & 0xFFu;
                ohp[j] = (int)(int16_t)(k2 & 0xFFFFu);
                ors[j] = (int)(int16_t)(k2 >> 16);
            }
#pragma unroll
            for (int j = 0; j < 4; j++) sl[j] = (cs[j] < CAP && snap_in(osb[j], v)) ? cs[j] : -1;
            for (uint64_t m = deadAny; m; m &= m - 1) {  // the view's dead units: a later list position wins
                const int ds = __builtin_ctzll(m);
                // from the pack, not by readlane of an inactive lane (poChunk's comment): the compiler sank
                // this wave's pack reads (cu, hp | res, snapshot byte) into the divergent item loop, so
                // lane ds's registers held a stale value whenever lane ds had no item (round 4's soak case)
                const uint32_t dcu = pk[ds], dkv = pk[64 + ds];
                const int dcell = uy(dcu) * W + ux(dcu);
                const int dh = (int)(int16_t)(dkv & 0xFFFFu), dr = (int)(int16_t)(dkv >> 16);
                const uint32_t dsb = pk[128 + ds] & 0xFFu;
                const bool mine = (deadM >> ds) & 1ull;
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (mine && dcell == 4 * c4 + j && ds > sl[j]) {
                        sl[j] = ds;
                        ocu[j] = dcu;
                        osb[j] = dsb;
                        ohp[j] = dh;
                        ors[j] = dr;
                    }
            }
            int vv[4][8];
#pragma unroll
            for (int j = 0; j < 4; j++) poPlanes(vv[j], sl[j] >= 0, ocu[j], osb[j], ohp[j], ors[j], cs[j] == WALL, v, mr, tr, x0 + j);
            const uint32_t base = (uint32_t)(v * D.C * HW + 4 * c4) * 4u;
#pragma unroll
            for (int k = 0; k < 8; k++) st4sc1(rs, base + (uint32_t)(k * HW) * 4u, vv[0][k], vv[1][k], vv[2][k], vv[3][k]);
        }
        wsync();
    }
    // the general form: any map, any unit count.  The last snapshot writer of every cell goes into a
    // per-cell scratch map (scell: slot + 1, the largest slot wins), the sight rows take several words
    // per row when W > 32.  delta (poDeltaShape maps, at most 64 units): as writeObsPOFast.
    DEV void writeObsPO(int slot, int p, bool delta = false) {
        if ((W & 3) == 0 && W <= 32 && H <= 32 && nu <= 64 && U.maxSight <= 15) {
            writeObsPOFast(slot, p, delta);
            return;
        }
        AB_SKIP(AB_PO_NOSCELL)
        for (int c = lid(); c < HW; c += 64) scell[c] = 0;
        const int NW = H * ((W + 31) >> 5);
        uint32_t* mineRows = vis;
        uint32_t* theirRows = vis + NW;
        for (int i = lid(); i < 2 * NW; i += 64) vis[i] = 0;
        wsync();
        const bool fastPaint = W <= 32 && U.maxSight <= 15;
        for (int o0 = 0; o0 < nu; o0 += 64) {
            const int o = o0 + lid();
            const bool in = o < nu && snap_in(snap[o], p);
            const uint32_t cu = in ? uc[o] : 0u;
            if (in) {
                AB_SKIP(AB_PO_NOSCELL)
                atomicMax(&scell[uy(cu) * W + ux(cu)], (uint32_t)(o + 1));
            }
            // visibility planes over the view's units at their current positions (dead ones
            // included: the view's list still holds them): own / other player's sight disks
            AB_SKIP(AB_PO_NOPAINT)
            {
                const bool painter = in && uplay(cu) >= 0;
                if (fastPaint) {
                    if (ballot(painter)) paintDisks(painter, cu, uplay(cu) == p ? mineRows : theirRows);
                } else if (painter) {
                    paintDisk(uplay(cu) == p ? mineRows : theirRows, cu);
                }
            }
        }
        wsync();
        int n = (HW + 3) >> 2;  // chunks to render: all, or the dirty list (delta maps have HW % 4 == 0)
        if (delta) {
            const int l = lid(), NCW = poChunkWords(HW);
            if (l < NCW) poDirty[l] = poPend[p * NCW + l];
            wsync();
            const int nu0 = hget(H_NU);  // the header holds the loaded unit count until store()
            if (l < nu || l < nu0) {
                const bool live = l < nu;
                const uint32_t cu = live ? uc[l] : 0u, sb = live ? (uint32_t)snap[l] : 0u;
                const uint32_t key = live ? (uint32_t)(uint16_t)hp[l] | ((uint32_t)(uint16_t)res[l] << 16) : 0u;
                poUnitChunks(poDirty, p, live && snap_in(sb, p), l < nu0, uy(cu) * W + ux(cu), uy(lcu) * W + ux(lcu), sb, key,
                             lsnap, lkey);
            }
            // sight rows (W <= 32: one word per row)
            for (int i = l; i < 2 * H; i += 64) poRowChunks(poDirty, vis[i] ^ poVis[p * 2 * H + i], (i < H ? i : i - H) * (W >> 2));
            wsync();
            // (a rolled loop of its own, not poListChunks' four unrolled rounds: this arm runs only for a
            // sight radius above 15, and its size counts in every kernel that holds it)
            n = 0;
            for (int c0 = 0; c0 < (HW >> 2); c0 += 64) {
                const int k = c0 + l;
                const bool dk = k < (HW >> 2) && ((poDirty[k >> 5] >> (k & 31)) & 1u);
                const uint64_t m = ballot(dk);
                if (dk) poList[n + lanes_below(m)] = (uint16_t)k;
                n += __popcll(m);
            }
            wsync();
        }
        int32_t* out = D.obs + (size_t)slot * D.C * HW;
        for (int it = lid(); it < n; it += 64) {
            const int c4 = delta ? (int)poList[it] : it;  // lane = 4 consecutive cells, dwordx4 per plane
            int sc[4];
#pragma unroll
            for (int j = 0; j < 4; j++) sc[j] = 4 * c4 + j < HW ? (int)scell[4 * c4 + j] - 1 : -1;
            uint32_t cu[4], sb[4];
            int ch[4], cr[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {  // branch-free: an empty cell reads slot 0 and is masked
                const int s = sc[j] >= 0 ? sc[j] : 0;
                cu[j] = uc[s];
                ch[j] = hp[s];
                cr[j] = res[s];
                sb[j] = snap[s];
            }
            const int cy = (4 * c4) / W, cx0 = (4 * c4) % W;  // W % 4 == 0 here, or one cell per lane below
            int v[4][8];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const bool in = 4 * c4 + j < HW;
                const int x = (W & 3) == 0 ? cx0 + j : (4 * c4 + j) % W, y = (W & 3) == 0 ? cy : (4 * c4 + j) / W;
                // (the sight bits as words whose bit 0 is the cell's: rows of several words when W > 32)
                poPlanes(v[j], sc[j] >= 0, cu[j], sb[j], ch[j], cr[j], in && cell[4 * c4 + j] == WALL, p,
                         in && seen(mineRows, x, y) ? 1u : 0u, in && seen(theirRows, x, y) ? 1u : 0u, 0);
            }
            if ((HW & 3) == 0) {
#pragma unroll
                for (int k = 0; k < 8; k++) st4<WT_POOBS>(out + k * HW + 4 * c4, v[0][k], v[1][k], v[2][k], v[3][k]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (4 * c4 + j < HW)
#pragma unroll
                        for (int k = 0; k < 8; k++) out[k * HW + 4 * c4 + j] = v[j][k];
            }
        }
        AB_SKIP(AB_PO_NORECORD)
        if (D.po_prev && poDeltaShape(H, W)) poRecord(p);
    }
    // the PO record of view p for the next write: this render's sight rows and the chunks of its units
    // that died (the compaction removes them before the next render)
    DEV void poRecord(int p) {
        const int l = lid(), NCW = poChunkWords(HW), SW = poSnapWords(CAP);
        int32_t* pr = D.po_prev + (size_t)g * D.po_words;
        for (int i = l; i < 2 * H; i += 64) pr[1 + SW + p * 2 * H + i] = (int32_t)vis[i];
        if (l < NCW) poDirty[l] = 0;
        wsync();
        for (int o = l; o < nu; o += 64) {
            const uint32_t cu = uc[o];
            if ((cu & UC_DEAD) && snap_in(snap[o], p)) poMarkCell(poDirty, uy(cu) * W + ux(cu));
        }
        wsync();
        if (l < NCW) pr[1 + SW + 4 * H + p * NCW + l] = (int32_t)poDirty[l];
        wsync();
    }
    // after the compaction: the snapshot bytes of the final slots and the views this launch rendered
    DEV void poRecordSnaps(uint32_t views) {
        int32_t* pr = D.po_prev + (size_t)g * D.po_words;
        // a render that kept its record in LDS (poLds) is followed, inside a multi-step launch, by an
        // iteration that reads the LDS copies: the global record is then stored at the last iteration only
        const bool glob = !iter || lastIt || !poLds;
        const uint32_t* sw = (const uint32_t*)snap;
        if (glob)
            for (int w = lid(); w < (nu + 3) / 4; w += 64) pr[1 + w] = (int32_t)sw[w];
        if (lid() == 0) {
            if (glob) pr[0] = (int32_t)views;
            hdr[HX_POVALID] = (int32_t)views;  // the record's LDS copy (multi-step launch)
        }
    }

    // ------------------------------------------------------------------ legal-action masks
    // JNIGridnetClient.getMasks (tests/JNIGridnetClient.java:210-223) + UnitAction.getValidActionArray
    // (rts/UnitAction.java:711-751) over Unit.getUnitActions(gs, 10) (rts/units/Unit.java:382-522).
    // farFromLanes: the range > 1 attack bits are left to farAttackBits (the caller's whole wave)
    DEV void unitMask(int s, uint32_t& w0, uint32_t& w1, uint32_t& w2, bool farFromLanes = false) const {
        uint64_t lo = 0;
        uint32_t hi = 0;
        auto setb = [&](int k) {
            if (k < 64) lo |= 1ull << k;
            else hi |= 1u << (k - 64);
        };
        const uint32_t cu = uc[s];
        const int x = ux(cu), y = uy(cu), typ = utyp(cu), pl = uplay(cu);
        const uint32_t fl = U.flags[typ];
        const int nt = NT, ctr = R / 2;
        const int atkBase = 1 + 6 + 16 + nt;
        setb(0);
        setb(1 + T_NONE);
        const bool canProduce = false;
        (void)canProduce;
        bool afford[MAX_PRODUCES];
#pragma unroll
        for (int i = 0; i < MAX_PRODUCES; i++) afford[i] = i < U.nprod[typ] && pres(pl) >= U.cost[U.prod[typ][i]];
        const int carried = res[s];
        const int r = U.range[typ];
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const int nx = x + dxo(d), ny = y + dyo(d);
            const int n = inb(nx, ny) ? cell[ny * W + nx] : WALL;
            if (n < CAP) {
                const uint32_t oc = uc[n];
                const int op = uplay(oc);
                const uint32_t ofl = U.flags[utyp(oc)];
                if ((fl & F_ATTACK) && r == 1 && op >= 0 && op != pl) {
                    setb(1 + T_ATTACK);
                    setb(atkBase + (ctr + dyo(d)) * R + (ctr + dxo(d)));
                }
                if (fl & F_HARVEST) {
                    if (carried == 0 && (ofl & F_RESOURCE)) {
                        setb(1 + T_HARVEST);
                        setb(1 + 6 + 4 + d);
                    }
                    if (carried > 0 && (ofl & F_STOCKPILE) && op == pl) {
                        setb(1 + T_RETURN);
                        setb(1 + 6 + 8 + d);
                    }
                }
            } else if (n == EMPTY) {
#pragma unroll
                for (int i = 0; i < MAX_PRODUCES; i++)
                    if (afford[i]) {
                        setb(1 + T_PRODUCE);
                        setb(1 + 6 + 12 + d);
                        setb(1 + 6 + 16 + U.prod[typ][i]);
                    }
                if (fl & F_MOVE) {
                    setb(1 + T_MOVE);
                    setb(1 + 6 + d);
                }
            }
        }
        if (!farFromLanes && (fl & F_ATTACK) && r > 1) {
            for (int dy = -r; dy <= r; dy++)
                for (int dx = -r; dx <= r; dx++) {
                    if (dx * dx + dy * dy > r * r || !inb(x + dx, y + dy)) continue;
                    const int n = cell[(y + dy) * W + x + dx];
                    if (n < CAP) {
                        const int op = uplay(uc[n]);
                        if (op >= 0 && op != pl) {
                            setb(1 + T_ATTACK);
                            setb(atkBase + (ctr + dy) * R + (ctr + dx));
                        }
                    }
                }
        }
        w0 = (uint32_t)lo;
        w1 = (uint32_t)(lo >> 32);
        w2 = hi;
    }
    // Wave-uniform per-type bit sets for maskBitsFast (bit t = unit type t has the property), the
    // produce lists as 8-bit type sets (type t's set in bits 8t..8t+7; mask bits ignore list order)
    // and, per player, the types whose cost the player's current resources cover.
    struct MaskTables {
        uint32_t attack1, attackFar, harvest, move, resource, stockpile, aff0, aff1;
        uint64_t prod;
    };
    DEV MaskTables maskTables() const {
        // the constant sets come with the unit-type table (host-computed, DevUtt::mt*); only the
        // affordability sets depend on the step (the players' resources now)
        const int t = lid();
        const bool ok = t < NT;
        const int cost = ok ? U.cost[t] : 0;
        MaskTables T;
        T.attack1 = uniu(U.mtAttack1);
        T.attackFar = uniu(U.mtAttackFar);
        T.harvest = uniu(U.mtHarvest);
        T.move = uniu(U.mtMove);
        T.resource = uniu(U.mtResource);
        T.stockpile = uniu(U.mtStockpile);
        T.prod = (uint64_t)uniu(U.mtProdLo) | ((uint64_t)uniu(U.mtProdHi) << 32);
        T.aff0 = (uint32_t)ballot(ok && pres0 >= cost);
        T.aff1 = (uint32_t)ballot(ok && pres1 >= cost);
        return T;
    }
    // unitMask's bits for range <= 1 units (the range > 1 attack window: farAttackBits) from the
    // tables: two LDS rounds (the 4 neighbour cells, then the units on them) instead of a dependent
    // read chain per neighbour and produce-list entry.  cu = the unit's core word, carried = its
    // resources.  Same bits as unitMask(s, ..., true).
    DEV void maskBitsFast(const MaskTables& T, uint32_t cu, int carried, uint32_t& w0, uint32_t& w1, uint32_t& w2) const {
        const int x = ux(cu), y = uy(cu), typ = utyp(cu), pl = uplay(cu);
        const int ctr = R / 2, atkBase = 1 + 6 + 16 + NT;
        int n[4];
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const int nx = x + dxo(d), ny = y + dyo(d);
            n[d] = inb(nx, ny) ? cell[ny * W + nx] : WALL;
        }
        uint32_t oc[4];
#pragma unroll
        for (int d = 0; d < 4; d++) oc[d] = n[d] < CAP ? uc[n[d]] : 0u;
        const bool atk = (T.attack1 >> typ) & 1u, harv = (T.harvest >> typ) & 1u, mov = (T.move >> typ) & 1u;
        const uint32_t canProd = (uint32_t)(T.prod >> (8 * typ)) & 0xFFu & (pl == 0 ? T.aff0 : T.aff1);
        uint64_t lo = 1ull | (1ull << (1 + T_NONE));
        uint32_t hi = 0;
        auto setb = [&](int k) {
            if (k < 64) lo |= 1ull << k;
            else hi |= 1u << (k - 64);
        };
#pragma unroll
        for (int d = 0; d < 4; d++) {
            if (n[d] < CAP) {
                const int op = uplay(oc[d]), ot = utyp(oc[d]);
                if (atk && op >= 0 && op != pl) {
                    setb(1 + T_ATTACK);
                    setb(atkBase + (ctr + dyo(d)) * R + (ctr + dxo(d)));
                }
                if (harv && carried == 0 && ((T.resource >> ot) & 1u)) {
                    setb(1 + T_HARVEST);
                    setb(1 + 6 + 4 + d);
                }
                if (harv && carried > 0 && ((T.stockpile >> ot) & 1u) && op == pl) {
                    setb(1 + T_RETURN);
                    setb(1 + 6 + 8 + d);
                }
            } else if (n[d] == EMPTY) {
                if (canProd) {
                    setb(1 + T_PRODUCE);
                    setb(1 + 6 + 12 + d);
                }
                if (mov) {
                    setb(1 + T_MOVE);
                    setb(1 + 6 + d);
                }
            }
        }
        // produce-type bits 23 + ut (below 64 for any table with <= 8 types)
        if (canProd && (n[0] == EMPTY || n[1] == EMPTY || n[2] == EMPTY || n[3] == EMPTY)) lo |= (uint64_t)canProd << (1 + 6 + 16);
        w0 = (uint32_t)lo;
        w1 = (uint32_t)(lo >> 32);
        w2 = hi;
    }
    // maskBitsFast's bits of ONE direction d (the lane of a quad that computes d; VERDICT r5 #4: the per-idle-unit
    // phases spread over lanes so that their instruction count falls): the unit-type and NONE bits, and what the
    // neighbour cell d holds — an enemy (range-1 attack), a resource (harvest), an own stockpile (return), an empty
    // cell (produce direction, move).  The quad's OR of its four results is maskBitsFast's, but for the produce-type
    // bits, which the caller adds once the OR shows a free cell (they need any of the four).  Every bit below the
    // attack window is in w0 (slot 1 + 6 + 12 + 3 = 22 < 32).
    DEV void maskBitsDir(const MaskTables& T, uint32_t cu, int carried, int d, uint32_t& w0, uint32_t& w1,
                         uint32_t& w2) const {
        const int x = ux(cu), y = uy(cu), typ = utyp(cu), pl = uplay(cu);
        const int ctr = R / 2, atkBase = 1 + 6 + 16 + NT;
        const int ddx = dxo(d), ddy = dyo(d), nx = x + ddx, ny = y + ddy;
        const int n = inb(nx, ny) ? cell[ny * W + nx] : WALL;
        const uint32_t oc = n < CAP ? uc[n] : 0u;
        const bool atk = (T.attack1 >> typ) & 1u, harv = (T.harvest >> typ) & 1u, mov = (T.move >> typ) & 1u;
        const uint32_t canProd = (uint32_t)(T.prod >> (8 * typ)) & 0xFFu & (pl == 0 ? T.aff0 : T.aff1);
        uint32_t lo = 1u | (1u << (1 + T_NONE)), mid = 0, hi = 0;
        if (n < CAP) {
            const int op = uplay(oc), ot = utyp(oc);
            if (atk && op >= 0 && op != pl) {
                lo |= 1u << (1 + T_ATTACK);
                const int k = atkBase + (ctr + ddy) * R + (ctr + ddx);
                if (k < 32) lo |= 1u << k;
                else if (k < 64) mid |= 1u << (k - 32);
                else hi |= 1u << (k - 64);
            }
            if (harv && carried == 0 && ((T.resource >> ot) & 1u)) lo |= (1u << (1 + T_HARVEST)) | (1u << (1 + 6 + 4 + d));
            if (harv && carried > 0 && ((T.stockpile >> ot) & 1u) && op == pl) lo |= (1u << (1 + T_RETURN)) | (1u << (1 + 6 + 8 + d));
        } else if (n == EMPTY) {
            if (canProd) lo |= (1u << (1 + T_PRODUCE)) | (1u << (1 + 6 + 12 + d));
            if (mov) lo |= (1u << (1 + T_MOVE)) | (1u << (1 + 6 + d));
        }
        w0 = lo;
        w1 = mid;
        w2 = hi;
    }
    // farAttackRows for the quad lane of direction d: its rows dy = d - ctr and d - ctr + 4 of the 2 ctr + 1 <= 7
    // (attack range <= 3: K <= 80), the same bits; the whole wave calls it
    DEV void farAttackRowsDir(bool far, uint32_t cu, int d, const uint32_t* rows, uint32_t& w0, uint32_t& w1,
                              uint32_t& w2) const {
        if (!ballot(far)) return;
        const int x = ux(cu), y = uy(cu), pl = uplay(cu);
        const int r = far ? U.range[utyp(cu)] : 0, ctr = R / 2, atkBase = 1 + 6 + 16 + NT;
        const uint32_t* er = rows + (far ? (1 - pl) * H : 0);
        uint64_t lo = 0;
        uint32_t hi = 0;
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int dy = d - ctr + 4 * j, yy = y + dy;
            if (!far || dy > ctr || dy < -r || dy > r || yy < 0 || yy >= H) continue;
            const uint64_t word = er[yy];
            uint64_t win = x >= r ? (word >> (x - r)) : (word << (r - x));  // bit j = column x - r + j
            // the disk's columns of row dy: |dx| <= half, half^2 + dy^2 <= r^2
            int half = 0;
            while (half < r && (half + 1) * (half + 1) + dy * dy <= r * r) half++;
            win &= ((2ull << (2 * half)) - 1ull) << (r - half);
            if (!win) continue;
            const int base = atkBase + (ctr + dy) * R + (ctr - r);
            if (base < 64) {
                lo |= win << base;
                if (base > 0) hi |= (uint32_t)(win >> (64 - base));
            } else {
                hi |= (uint32_t)(win << (base - 64));
            }
            lo |= 1ull << (1 + T_ATTACK);
        }
        w0 |= (uint32_t)lo;
        w1 |= (uint32_t)(lo >> 32);
        w2 |= hi;
    }
    static DEV uint32_t quadOr(uint32_t v) {  // OR over the lane's quad (DPP quad_perm; whole wave)
        LANE_AUDIT_WAVE(2);
        v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);  // quad_perm [1,0,3,2]
        v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);  // quad_perm [2,3,0,1]
        return v;
    }
    // maskBitsFast + farAttackRows of every idle unit (si >= 0), four lanes per unit: the units' words go to LDS
    // in rank order (16 per pass), lane 4 q + d computes direction d (and rows d - ctr, d - ctr + 4 of the
    // ranged window) of unit q, the quad ORs its words, and the unit's own lane reads them back — the same bits
    // as one lane per unit, in about a quarter of the instructions.  rows complete (wsync'd);
    // rseq words 16..63 are scratch here.  Whole wave.
    DEV void maskBitsQuads(const MaskTables& T, int si, uint32_t cu, int carried, const uint32_t* rows, uint32_t& w0,
                           uint32_t& w1, uint32_t& w2, uint32_t* qb /* [16][3] scratch words */) {
        const int l = lid();
        const uint64_t m = ballot(si >= 0);
        const int RI = __popcll(m), r = lanes_below(m);
        const int q = l >> 2, d = l & 3;
        for (int p0 = 0; p0 < RI; p0 += 16) {
            const bool mine = si >= 0 && r >= p0 && r < p0 + 16;
            if (mine) {
                qb[3 * (r - p0)] = cu;
                qb[3 * (r - p0) + 1] = (uint32_t)carried;
            }
            wsync();
            const bool qa = p0 + q < RI;
            uint32_t qcu = 0, v0 = 0, v1 = 0, v2 = 0;
            if (qa) {
                qcu = qb[3 * q];
                maskBitsDir(T, qcu, (int)qb[3 * q + 1], d, v0, v1, v2);
            }
            farAttackRowsDir(qa && ((T.attackFar >> utyp(qcu)) & 1u), qcu, d, rows, v0, v1, v2);
            v0 = quadOr(v0);
            v1 = quadOr(v1);
            v2 = quadOr(v2);
            // produce-type bits 23 + ut, when a direction of the quad found a free cell (produce direction bits)
            const uint32_t canProd =
                (uint32_t)(T.prod >> (8 * utyp(qcu))) & 0xFFu & (uplay(qcu) == 0 ? T.aff0 : T.aff1);
            if (((v0 >> (1 + 6 + 12)) & 0xFu) != 0u) v0 |= canProd << (1 + 6 + 16);
            wsync();  // every lane of a quad has read its entry
            if (qa && d == 0) {
                qb[3 * q] = v0;
                qb[3 * q + 1] = v1;
                qb[3 * q + 2] = v2;
            }
            wsync();
            if (mine) {
                w0 = qb[3 * (r - p0)];
                w1 = qb[3 * (r - p0) + 1];
                w2 = qb[3 * (r - p0) + 2];
            }
            wsync();  // read before the next pass rewrites the entries
        }
    }
    // The range > 1 attack bits of unitMask (Unit.java:424-434: every enemy unit within the disk) for
    // lanes with far = true, from the unit list held one unit per lane (cuLane = unit core word of
    // lane j, all units in one wave, none dead): one pass over the live owned units instead of a
    // (2r+1)^2 cell scan per ranged unit — the same set, as a cell holds at most one unit.  Whole wave.
    DEV void farAttackBits(bool far, uint32_t cu, uint32_t cuLane, uint64_t owned, uint32_t& w0, uint32_t& w1,
                           uint32_t& w2) const {
        if (!ballot(far)) return;
        const int x = ux(cu), y = uy(cu), pl = uplay(cu);
        const int r = far ? U.range[utyp(cu)] : 0, ctr = R / 2, atkBase = 1 + 6 + 16 + NT;
        uint64_t lo = 0;
        uint32_t hi = 0;
        for (uint64_t m = owned; m; m &= m - 1) {
            const uint32_t cj = uniu((uint32_t)rl((int)cuLane, __builtin_ctzll(m)));
            const int dx = ux(cj) - x, dy = uy(cj) - y;
            if (far && uplay(cj) != pl && dx * dx + dy * dy <= r * r) {
                const int k = atkBase + (ctr + dy) * R + (ctr + dx);
                if (k < 64) lo |= 1ull << k;
                else hi |= 1u << (k - 64);
                lo |= 1ull << (1 + T_ATTACK);
            }
        }
        w0 |= (uint32_t)lo;
        w1 |= (uint32_t)(lo >> 32);
        w2 |= hi;
    }
    // farAttackBits from per-player unit row bitmaps (rows[p * H + y] bit x = a unit of player p at
    // (x, y); W <= 32): each far lane reads the 2r + 1 enemy rows around it and keeps the bits inside
    // the disk.  Whole wave; rows complete (after a wsync).
    DEV void farAttackRows(bool far, uint32_t cu, const uint32_t* rows, uint32_t& w0, uint32_t& w1, uint32_t& w2) const {
        if (!ballot(far)) return;
        const int x = ux(cu), y = uy(cu), pl = uplay(cu);
        const int r = far ? U.range[utyp(cu)] : 0, ctr = R / 2, atkBase = 1 + 6 + 16 + NT;
        const uint32_t* er = rows + (far ? (1 - pl) * H : 0);
        uint64_t lo = 0;
        uint32_t hi = 0;
#pragma unroll
        for (int dy = -ctr; dy <= ctr; dy++) {
            const int yy = y + dy;
            if (!far || dy < -r || dy > r || yy < 0 || yy >= H) continue;
            const uint64_t word = er[yy];
            uint64_t win = x >= r ? (word >> (x - r)) : (word << (r - x));  // bit j = column x - r + j
            uint64_t disk = 0;
#pragma unroll
            for (int j = 0; j <= 2 * ctr; j++)
                if (j <= 2 * r && (j - r) * (j - r) + dy * dy <= r * r) disk |= 1ull << j;
            win &= disk;
            if (!win) continue;
            const int base = atkBase + (ctr + dy) * R + (ctr - r);
            if (base < 64) {
                lo |= win << base;
                if (base > 0) hi |= (uint32_t)(win >> (64 - base));
            } else {
                hi |= (uint32_t)(win << (base - 64));
            }
            lo |= 1ull << (1 + T_ATTACK);
        }
        w0 |= (uint32_t)lo;
        w1 |= (uint32_t)(lo >> 32);
        w2 |= hi;
    }
    // Park each idle unit's 79-bit mask in its unused assignment words (at/as/ua low bits).
    // pset: bit p = park the masks of player p's idle units (both players in one pass for self-play)
    DEV void stashMasks(int pset) {
        for (int o = lid(); o < nu; o += 64) {
            const uint32_t c = uc[o];
            const int op = uplay(c);
            if ((c & UC_DEAD) || op < 0 || !((pset >> op) & 1) || (ua[o] & UA_PRESENT)) continue;
            uint32_t w0, w1, w2;
            unitMask(o, w0, w1, w2);
            at[o] = (int32_t)w0;
            as[o] = (int32_t)w1;
            ua[o] = w2 & 0xFFFFu;
        }
    }
    DEV void cellMaskBits(int c, int p, uint64_t& lo, uint32_t& hi) const {
        lo = 0;
        hi = 0;
        if (c >= HW) return;
        const int s = cell[c];
        if (s < CAP && uplay(uc[s]) == p && !(ua[s] & UA_PRESENT)) {
            lo = (uint64_t)(uint32_t)at[s] | ((uint64_t)(uint32_t)as[s] << 32);
            hi = ua[s] & 0xFFFFu;
        }
    }
    static DEV uint32_t bits16(uint64_t lo, uint32_t hi, int k) {  // bits k..k+15 of a 96-bit vector
        uint64_t v;
        if (k == 0) v = lo;
        else if (k < 64) v = (lo >> k) | ((uint64_t)hi << (64 - k));
        else v = (uint64_t)hi >> (k - 64);
        return (uint32_t)v & 0xFFFFu;
    }
    static DEV uint32_t expand4(uint32_t b) { return ((b & 0xFu) * 0x00204081u) & 0x01010101u; }
    // one 16-byte chunk j of the [HW][K] byte mask of player p, from the parked per-unit bits
    DEV uint4 maskChunk(int j, int p) const {
        const int o0 = 16 * j;
        const int cA = o0 / K, kA = o0 - cA * K;
        uint64_t lo;
        uint32_t hi;
        cellMaskBits(cA, p, lo, hi);
        uint32_t b = bits16(lo, hi, kA);
        const int nA = K - kA;
        if (nA < 16) {
            b &= (1u << nA) - 1u;
            cellMaskBits(cA + 1, p, lo, hi);
            b |= (bits16(lo, hi, 0) << nA) & 0xFFFFu;
        }
        uint4 v;
        v.x = expand4(b);
        v.y = expand4(b >> 4);
        v.z = expand4(b >> 8);
        v.w = expand4(b >> 12);
        return v;
    }
    DEV bool ownIdleAt(int c, int p) const {
        const int s = c < HW ? cell[c] : EMPTY;
        return s < CAP && uplay(uc[s]) == p && !(ua[s] & UA_PRESENT);
    }
    // The mask rows of the game's external slots (slot0 + i is player pl[i]'s view).  Full mode writes
    // all H*W*K bytes per slot; delta mode (the buffer holds this handle's previous masks) rewrites
    // only the 16-byte chunks overlapping a cell that has, or had at the previous write, an own idle
    // unit — the buffer ends up identical.  The dirty cells of both slots are gathered into one list
    // and their chunks are spread over the lanes, so a typical step is a single parallel pass.
    DEV void writeMasks(int slot0, int nslots, int pl0, int pl1) {
        const int total = HW * K;
        const int MW = maskWords(HW);
        const bool delta = D_ON(mask_delta) && (total & 15) == 0;
        uint32_t* pg = prevG();
        const int l = lid();
        if (delta && nu <= 64 && nslots * MW <= 64 && writeMasksUnits(slot0, nslots, pl0, pl1)) return;
        int nlist = 0;
        for (int i = 0; i < nslots; i++) {
            const int p = i ? pl1 : pl0;
            const int slot = slot0 + i;
            for (int c0 = 0; c0 < HW; c0 += 64) {
                const uint64_t m = ballot(ownIdleAt(c0 + l, p));
                const int w = c0 >> 5;
                const uint32_t mine = l == 0 ? (uint32_t)m : (uint32_t)(m >> 32);
                if (l < 2 && w + l < MW) {
                    if (D_HAS(source)) D.source[(size_t)slot * MW + w + l] = mine;
                    if (lastIt) pg[p * MW + w + l] = mine;
                }
                if (delta) {
                    const uint64_t old = (uint64_t)mprev[p * MW + w] | (w + 1 < MW ? (uint64_t)mprev[p * MW + w + 1] << 32 : 0ull);
                    const uint64_t dirty = old | m;
                    const int n = __popcll(dirty);
                    if (n) {
                        if (nlist + n > 64) {
                            flushDirty(nlist, slot0, pl0, pl1);
                            nlist = 0;
                        }
                        if ((dirty >> l) & 1ull) rslot[nlist + lanes_below(dirty)] = (uint16_t)((i << 15) | (c0 + l));
                        nlist += n;
                    }
                }
                if (l < 2 && w + l < MW) mprev[p * MW + w + l] = mine;  // after the read: a multi-step launch's next base
            }
        }
        MPHASE(11);
        if (delta) {
            if (nlist) flushDirty(nlist, slot0, pl0, pl1);
            return;
        }
        for (int i = 0; i < nslots; i++) {
            const int p = i ? pl1 : pl0;
            uint8_t* out = D.masks + (size_t)(slot0 + i) * total;
            if ((total & 15) == 0) {
                for (int j = l; j < total / 16; j += 64) {
                    const uint4 v = maskChunk(j, p);
                    st4<WT_FULLMASK>(out + 16 * j, (int)v.x, (int)v.y, (int)v.z, (int)v.w);
                }
            } else {
                for (int o = l; o < total; o += 64) {
                    const int c = o / K, k = o - c * K;
                    uint64_t lo;
                    uint32_t hi;
                    cellMaskBits(c, p, lo, hi);
                    out[o] = (uint8_t)(k < 64 ? ((lo >> k) & 1u) : ((hi >> (k - 64)) & 1u));
                }
            }
        }
    }
    // Delta form with all units in one wave: the new row sets come from the units (one atomicOr per
    // idle unit), old|new per bit word gives the dirty cells, and a wave prefix sum lists them.
    // Returns false (nothing written) when the list would exceed 64 cells.
    DEV bool writeMasksUnits(int slot0, int nslots, int pl0, int pl1) {
        const int MW = maskWords(HW), NW = nslots * MW;
        const int l = lid();
        uint32_t* nb = (uint32_t*)rseq;  // cycle() scratch, free here: [slot i][MW] new bits
        if (l < NW) nb[l] = 0;
        wsync();
        if (l < nu) {
            const uint32_t cu = uc[l];
            if (!(cu & UC_DEAD) && !(ua[l] & UA_PRESENT)) {
                const int op = uplay(cu), c = uy(cu) * W + ux(cu);
                if (op >= 0 && op == pl0) atomicOr(&nb[c >> 5], 1u << (c & 31));
                if (nslots > 1 && op >= 0 && op == pl1) atomicOr(&nb[MW + (c >> 5)], 1u << (c & 31));
            }
        }
        wsync();
        uint32_t cur = 0, old = 0;
        int i = 0, w = 0;
        if (l < NW) {
            i = l >= MW;
            w = l - i * MW;
            cur = nb[l];
            old = mprev[(i ? pl1 : pl0) * MW + w];
        }
        const uint32_t dirty = cur | old;
        const int n = __popc(dirty);
        const int incl = wave_incl_sum(n);
        const int total = rl(incl, 63);
        if (total > 64) return false;
        if (l < NW) {
            if (D_HAS(source)) D.source[(size_t)(slot0 + i) * MW + w] = cur;
            if (lastIt) prevG()[(i ? pl1 : pl0) * MW + w] = cur;  // the next launch's copy
            mprev[(i ? pl1 : pl0) * MW + w] = cur;
        }
        if (total == 0) return true;
        int k = incl - n;
        for (uint32_t d = dirty; d; d &= d - 1) rslot[k++] = (uint16_t)((i << 15) | (32 * w + __builtin_ctz(d)));
        flushDirty(total, slot0, pl0, pl1);
        return true;
    }
    // One cell's K-byte mask record (byte k = bit k of lo:hi) at dst, byte-exact: up to 3 head bytes to
    // reach dword alignment, whole dwords (dwordx4 / dwordx3 stores, 4-byte aligned), then the tail
    // bytes — neighbouring records written by other lanes are never touched.
    DEV void storeRecord(uint8_t* dst, uint64_t lo, uint32_t hi) const {
        const int head = (int)((4u - ((uint32_t)(uintptr_t)dst & 3u)) & 3u);
#pragma unroll
        for (int i = 0; i < 3; i++)
            if (i < head) dst[i] = (uint8_t)((lo >> i) & 1u);
        // bits head.. as a 96-bit value v0:v1:v2
        const uint64_t sl = (lo >> head) | (head ? ((uint64_t)hi << (64 - head)) : 0ull);
        const uint32_t sh = hi >> head;
        const uint32_t v[3] = {(uint32_t)sl, (uint32_t)(sl >> 32), sh};
        const int nd = (K - head) >> 2;  // whole dwords
        uint32_t* dw = (uint32_t*)(dst + head);
        auto nib = [&](int k) -> uint32_t { return expand4(v[k >> 3] >> (4 * (k & 7))); };
        if (K == 79) {  // nd == 19 for every head
#pragma unroll
            for (int q = 0; q < 4; q++) {
                st4u<WT_MASK>(dw + 4 * q, (int)nib(4 * q), (int)nib(4 * q + 1), (int)nib(4 * q + 2), (int)nib(4 * q + 3));
            }
            st3u<WT_MASK>(dw + 16, (int)nib(16), (int)nib(17), (int)nib(18));
        } else {
            for (int k = 0; k < nd; k++) dw[k] = nib(k);
        }
        const int t0 = head + 4 * nd;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const int b = t0 + i;
            if (b < K) dst[b] = (uint8_t)((b < 64 ? (lo >> b) : (uint64_t)(hi >> (b - 64))) & 1u);
        }
    }
    // The K = 79 mask records of the lanes with si >= 0 (slot index si, cell c, mask bits w0:w1:w2) stored
    // lane-parallel: the records are listed in LDS (rseq words 16..63, 12 records of 4 words), then five lanes
    // store each record — lanes 0..3 of it 16 bytes each, lane 4 the last 12 — from the record's 16-bit
    // field at their offset (byte k = bit k, expand4), and lanes 0..2 one of its 3 head / tail bytes each.
    // The record's bytes are storeRecord's; a lane storing its own record (storeRecord) spent ~85 VALU
    // instructions on it, all of which the other lanes waited through (round 5: ~35 for 12 records).
    // `mrs` covers the game's records from `mbase`; the caller's rseq words 0..15 are not touched.
    DEV void storeRecordsLanes(int si, int c, uint32_t w0, uint32_t w1, uint32_t w2, __amdgpu_buffer_rsrc_t mrs,
                               const uint8_t* mbase, int total) const {
        const uint64_t m = ballot(si >= 0);
        const int R = __popcll(m);
        if (R == 0) return;
        const int l = lid();
        const int r = lanes_below(m);
        uint32_t* rb = (uint32_t*)rseq + 16;
        const int tr = (l * 13) >> 6, q = l - 5 * tr;  // record tr of a pass, its part q (lanes 0..59)
        const int sel = q >> 1;                         // words sel, sel + 1 hold the part's bits
        const uint32_t mbLo = (uint32_t)(uintptr_t)mbase;
        for (int p0 = 0; p0 < R; p0 += 12) {
            if (si >= 0 && r >= p0 && r < p0 + 12) {
                uint32_t* e = rb + 4 * (r - p0);
                e[0] = w0;
                e[1] = w1;
                e[2] = w2;
                e[3] = ((uint32_t)si << 16) | (uint32_t)c;
            }
            wsync();
            if (l < 60 && p0 + tr < R) {
                const uint32_t* e = rb + 4 * tr;
                const uint32_t lo = e[sel], hi = e[sel + 1], meta = e[3];
                const uint32_t s = (meta >> 16) * (uint32_t)total + (meta & 0xFFFFu) * 79u;
                const uint32_t h = (0u - (mbLo + s)) & 3u;  // head bytes before the first aligned dword
                // bits h + 16 q .. + 15 of the record: the low half of the funnel shift of (hi:lo)
                const uint32_t x = __builtin_amdgcn_alignbit(hi, lo, h + 16u * (uint32_t)(q & 1));
                const int d0 = (int)expand4(x), d1 = (int)expand4(x >> 4), d2 = (int)expand4(x >> 8),
                          d3 = (int)expand4(x >> 12);
                const int off = (int)(s + h) + 16 * q;
                if (q < 4) {
                    const i32x4v v = {d0, d1, d2, d3};
                    __builtin_amdgcn_raw_buffer_store_b128(v, mrs, off, 0, SC1_MASK ? 16 : 0);
                } else {
                    typedef int32_t i32x3v __attribute__((ext_vector_type(3)));
                    const i32x3v v = {d0, d1, d2};
                    __builtin_amdgcn_raw_buffer_store_b96(v, mrs, off, 0, SC1_MASK ? 16 : 0);
                }
                if (q < 3) {  // byte q of the 3 outside the 19 dwords: head byte q, else tail byte 76 + q
                    const bool head = (uint32_t)q < h;
                    const uint32_t b = head ? (uint32_t)q : 76u + (uint32_t)q;
                    const uint32_t v = ((head ? e[0] : (e[2] >> 12)) >> q) & 1u;
                    __builtin_amdgcn_raw_buffer_store_b8((char)v, mrs, (int)(s + b), 0, SC1_MASK ? 16 : 0);
                }
            }
            wsync();
        }
    }
    // Delta mask writes with every unit in one wave (nu <= 64, K <= 96): each own idle unit's lane
    // computes its Unit.getUnitActions mask bits in registers and stores its whole record (and, fused
    // policy, its action row) itself; cells that held an idle unit at the previous write and hold none
    // now get a zero record (and a zero row).  Same buffer contents as stashMasks + writeMasks.
    DEV void writeMasksLanes(int slot0, int nslots, int pl0, int pl1) {
        const int MW = maskWords(HW), NW = nslots * MW;
        const int l = lid();
        const int total = HW * K;
        uint32_t* nb = (uint32_t*)rseq;  // cycle() scratch, free here: [slot i][MW] new bits
        if (l < NW) nb[l] = 0;
        // per-player unit row bitmaps for the range > 1 attack bits (rslot scratch, free here)
        // (partially observable games on maps of 16 to 32 columns: in the tail of `scell`, free during the masks —
        // the general render's scratch map is done with, and a helper wave's packs and cell map end at word 896 of
        // 32x32's 1,024 (round 6: c5's ranged units had taken farAttackBits' walk over every live unit))
        const bool rowS = W <= 32 && 2 * H <= 32;
        const bool rowP = !rowS && po && W <= 32 && W >= 16 && 2 * H <= 64;
        uint32_t* rows = rowS ? (uint32_t*)rslot : rowP ? scell + (HW - 2 * H) : nullptr;
        const bool rowB = rowS || rowP;
        if (rowB && l < 2 * H) rows[l] = 0;
        int si = -1;  // slot index of this lane's unit record, -1 = none
        uint32_t cu = 0;
        if (l < nu) {
            cu = uc[l];
            if (!(cu & UC_DEAD) && !(ua[l] & UA_PRESENT)) {
                const int op = uplay(cu);
                if (op >= 0 && op == pl0) si = 0;
                else if (nslots > 1 && op >= 0 && op == pl1) si = 1;
            }
        }
        const int c = uy(cu) * W + ux(cu);
        wsync();
        if (si >= 0) atomicOr(&nb[si * MW + (c >> 5)], 1u << (c & 31));
        if (rowB && l < nu && !(cu & UC_DEAD) && uplay(cu) >= 0) atomicOr(&rows[uplay(cu) * H + uy(cu)], 1u << ux(cu));
        AB_ON(AB_MASKSETUP, ablMaskSetup(nb, NW, MW, rows, rowB, nslots > 1, pl0, pl1));
        uint32_t w0 = 0, w1 = 0, w2 = 0;
        {
            MPHASE(16);
            const MaskTables T = maskTables();
            AB_ON(AB_TABLES, ablTables());
            MPHASE(17);
            const int carried = l < nu ? res[l] : 0;
            // four lanes per idle unit wherever the row bitmaps exist: its 48 scratch words are rseq words 16..63
            // while the new row sets nb take <= 16 words, else (32x32 views) the 48 words of scell's tail below
            // the rows (past a helper wave's packs and cell map, which end at word 896 of 1,024)
            uint32_t* const qb = NW <= 16 ? (uint32_t*)rseq + 16 : (rowP && HW - 2 * H - 48 >= 896) ? rows - 48 : nullptr;
            if (rowB && qb) {
                wsync();
                maskBitsQuads(T, si, cu, carried, rows, w0, w1, w2, qb);
            } else {
                if (si >= 0) maskBitsFast(T, cu, carried, w0, w1, w2);
                MPHASE(18);
                const bool far = si >= 0 && ((T.attackFar >> utyp(cu)) & 1u);
                if (rowB) {
                    wsync();
                    farAttackRows(far, cu, rows, w0, w1, w2);
                } else {
                    farAttackBits(far, cu, cu, ballot(l < nu && !(cu & UC_DEAD) && uplay(cu) >= 0), w0, w1, w2);
                }
            }
            if (rowB) AB_ON(AB_MASKBITS, ablMaskBits(T, si, cu, carried, rows, qb));
            MPHASE(19);
        }
        wsync();
        MPHASE(12);
        uint32_t cur = 0, old = 0;
        int i = 0, w = 0;
        if (l < NW) {
            i = l >= MW;
            w = l - i * MW;
            cur = nb[l];
            old = mprev[(i ? pl1 : pl0) * MW + w];
            if (D_HAS(source)) D.source[(size_t)(slot0 + i) * MW + w] = cur;
            if (lastIt) prevG()[(i ? pl1 : pl0) * MW + w] = cur;  // the next launch's copy
            mprev[(i ? pl1 : pl0) * MW + w] = cur;  // the next iteration's base (multi-step launch)
        }
        const bool pol = D_HAS(pol_actions) && D_ON(pol_delta);
        // forward the sampled rows of a self-play game (read by selfPlayFast next launch); K - 23 - NT
        // attack slots fit packFwd's 7-bit field
        const bool fwdW = pol && nslots == 2 && K - 23 - NT <= 126;
        const uint8_t* mbase = D.masks + (size_t)slot0 * total;  // this game's records
        const __amdgpu_buffer_rsrc_t mrs = bufRsrc((void*)mbase, (uint32_t)(nslots * total));
        // the kernel's full policy pass (writePolicyAll, no delta base) reads the parked bits
        if (si >= 0 && D_HAS(pol_actions) && !(D_ON(pol_delta) && D_ON(mask_delta) && (total & 15) == 0)) {
            at[l] = (int32_t)w0;
            as[l] = (int32_t)w1;
            ua[l] = w2 & 0xFFFFu;
        }
        if (recOut && si < 0) recOut[l] = ~0u;  // (no record from this lane)
        // the records stored lane-parallel (storeRecordsLanes) rather than each by its own lane
        const bool lanePar = !recOut && K == 79 && NW <= 16;
        if (lanePar) {
            AB_SKIP(AB_SKIP_RECORD)
            storeRecordsLanes(si, c, w0, w1, w2, mrs, mbase, total);
            AB_ON(AB_RECORD, storeRecordsLanes(launder(si), launder(c), launder(w0), launder(w1), launder(w2), mrs, mbase, total));
        }
        if (si >= 0) {
            const int slot = slot0 + si;
            const uint64_t lo = (uint64_t)w0 | ((uint64_t)w1 << 32);
            if (recOut) {  // the helper expands and stores it (storeRecordsHelp)
                recOut[l] = ((uint32_t)si << 16) | (uint32_t)c;
                recOut[64 + l] = w0;
                recOut[128 + l] = w1;
                recOut[192 + l] = w2;
            } else if (lanePar) {
            } else
            AB_SKIP(AB_SKIP_RECORD)
            storeRecord(D.masks + (size_t)slot * total + (size_t)c * K, lo, w2);
            AB_ON(AB_RECORD, storeRecord(D.masks + (size_t)slot * total + (size_t)c * K, launder(lo), launder(w2)));
            MPHASE(13);
            if (pol) {
                int32_t a[7];
                AB_ON(AB_POLICY, ablSample(slot, lo, w2, c));
                uint32_t pk;
                sampleBitsRaw(D.pol_seed, polStep, D.pol_slot_base + (uint32_t)slot, NT, K, (lo >> 1) | ((uint64_t)w2 << 63),
                              (uint64_t)(w2 >> 1), c, a, &pk);
                if (recOut) {
                    recOut[256 + l] = pk;
                } else {
                    int32_t* dst = D.pol_actions + ((size_t)slot * HW + c) * 7;
                    st4u<WT_MASK>(dst, a[0], a[1], a[2], a[3]);
                    st3u<WT_MASK>(dst + 4, a[4], a[5], a[6]);
                }
                if (fwdW) {
                    // packFwd(a): the next launch decodes from it, and so does the next iteration of a multi-step
                    // launch (the steady instance's takes the row decoded: writeMasksSteady)
                    if (lastIt) st1<WT_STATE>(st() + stateFwdOff(CAP, HW) + l, (int32_t)pk);  // the next launch's
                    lfwd = pk;
                }
            }
        }
        fwdWritten = fwdW;
        MPHASE(14);
        // cells whose idle unit is gone: zero record + zero row
        const uint32_t gone = old & ~cur;
        const int n = __popc(gone);
        const int incl = wave_incl_sum(n);
        const int ngone = rl(incl, 63);
        if (recOut) {  // the vacated cells go to the helper too (up to 64 of them; more: stored here below)
            uint16_t* gl = (uint16_t*)(recOut + 5 * 64 + 1);
            if (ngone <= 64) {
                int k = incl - n;
                for (uint32_t d = gone; d; d &= d - 1, k++) gl[k] = (uint16_t)((i << 15) | (32 * w + __builtin_ctz(d)));
            }
            if (l == 0) recOut[5 * 64] = (1u << 31) | (uint32_t)(ngone <= 64 ? ngone : 0);  // (bit 31: records valid)
            if (ngone <= 64) {
                wsync();
                return;
            }
        }
        if (ngone == 0) {
            wsync();
            return;
        }
        AB_TWICE(AB_GONE)
        for (int b0 = 0; b0 < ngone; b0 += 64) {  // rslot holds 64 list entries at a time
            wsync();
            int k = incl - n;
            for (uint32_t d = gone; d; d &= d - 1, k++)
                if (k >= b0 && k < b0 + 64) rslot[k - b0] = (uint16_t)((i << 15) | (32 * w + __builtin_ctz(d)));
            wsync();
            if (b0 + l < ngone) {
                const uint32_t e = rslot[l];
                const int slot = slot0 + (int)(e >> 15), cz = (int)(e & 0x7FFFu);
                storeRecord(D.masks + (size_t)slot * total + (size_t)cz * K, 0ull, 0u);
                if (pol) {
                    int32_t* dst = D.pol_actions + ((size_t)slot * HW + cz) * 7;
                    st4u<WT_MASK>(dst, 0, 0, 0, 0);
                    st3u<WT_MASK>(dst + 4, 0, 0, 0);
                }
            }
        }
        wsync();
    }
    static DEV int rowInclSum(int v) {  // wave_incl_sum inside each 16-lane row (its first four steps; whole wave)
        LANE_AUDIT_WAVE(2);
        v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, false);  // row_shr:1
        v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, false);  // row_shr:2
        v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, false);  // row_shr:4
        v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, false);  // row_shr:8
        return v;
    }
    // writeMasksLanes of the steady instance (self-play on 16x16, K = 79, delta masks and delta policy
    // rows, nu <= 64): the same buffer contents from one list of quads.  An entry of the list (qb: 16 of 3 words a
    // pass, rseq words 16..63) is an own idle unit — its core word, its resources | its lane << 16 — or, after the
    // units, a cell whose idle unit is gone, as the core word of a unit of that player on that cell.  Lane 4 q + d
    // computes direction d of entry q (maskBitsDir, farAttackRowsDir) and quadOr leaves the row on the quad's four
    // lanes — zero for a vacated cell, whose lanes compute nothing.  From its registers lane d then stores 16 bytes
    // of the record, lane 3 the last 12 as well and lanes 0..2 one head / tail byte each (storeRecordsLanes' bytes);
    // lane 0 samples the row, stores it (a zero row for a vacated cell), on the launch's last step the forwarded word
    // at the unit's lane index, and posts the decoded word in the entry's third word, where the unit's own lane
    // takes it (lfwd) after the pass.  More than 16 entries take further passes.  Whole wave.
    DEV void writeMasksSteady(int slot0) {
        constexpr int MW = 8, NW = 16;  // maskWords(16 * 16), both slots
        const int l = lid();
        const int total = HW * K;
        uint32_t* nb = (uint32_t*)rseq;          // [slot][MW] new row sets
        uint32_t* qb = (uint32_t*)rseq + 16;      // the list
        uint32_t* rows = (uint32_t*)rslot;        // per-player unit row bitmaps (farAttackRowsDir)
        if (l < NW) nb[l] = 0;
        int si = -1;
        uint32_t cu = 0;
        if (l < nu) {
            cu = uc[l];
            if (!(cu & UC_DEAD) && !(ua[l] & UA_PRESENT)) si = uplay(cu);  // (slot i is player i's; -1: a resource)
        }
        const int c = uy(cu) * W + ux(cu);
        const uint64_t im = ballot(si >= 0);
        const int RI = __popcll(im), r = lanes_below(im);
        idleOwn = RI;
        // the row bitmaps only when an idle unit attacks at range > 1 (farAttackRowsDir returns at once otherwise)
        const bool rowF = ballot(si >= 0 && ((uniu(U.mtAttackFar) >> utyp(cu)) & 1u)) != 0;
        if (rowF && l < 2 * H) rows[l] = 0;
        wsync();
        if (si >= 0) atomicOr(&nb[si * MW + (c >> 5)], 1u << (c & 31));
        if (rowF && l < nu && !(cu & UC_DEAD) && uplay(cu) >= 0) atomicOr(&rows[uplay(cu) * H + uy(cu)], 1u << ux(cu));
        AB_ON(AB_MASKSETUP, ablMaskSetup(nb, NW, MW, rows, rowF, true, 0, 1));  // (slot i is player i's)
        MPHASE(16);
        const MaskTables T = maskTables();
        AB_ON(AB_TABLES, ablTables());
        MPHASE(17);
        const uint32_t own = ((uint32_t)(l < nu ? res[l] : 0) & 0xFFFFu) | (uint32_t)l << 16;
        wsync();
        // the row sets: the source bits, the next step's / launch's base, the cells whose idle unit is gone
        uint32_t gone = 0;
        if (l < NW) {
            const uint32_t cur = nb[l], old = mprev[l];  // (player i's words are slot i's)
            D.source[(size_t)slot0 * MW + l] = cur;
            if (lastIt) prevG()[l] = cur;
            mprev[l] = cur;
            gone = old & ~cur;
        }
        const int n = __popc(gone);
        const int incl = rowInclSum(n);  // (lanes 0..15 hold the words)
        const int NR = RI + rl(incl, 15);
        AB_ON(AB_GONE, keepv(rl(rowInclSum(launder(n)), 15)));  // the scan alone: the zero records ride the unit pass
        MPHASE(12);
        const uint32_t mbLo = (uint32_t)(uintptr_t)(D.masks + (size_t)slot0 * total);
        const __amdgpu_buffer_rsrc_t mrs = bufRsrc((void*)(D.masks + (size_t)slot0 * total), (uint32_t)(2 * total));
        const int q = l >> 2, d = l & 3;
        // the quad's lanes store the record (w0:w1:w2) of the entry with core word ecu
        auto storeQuad = [&](uint32_t ecu, uint32_t w0, uint32_t w1, uint32_t w2) {
            const uint32_t s = (uint32_t)uplay(ecu) * (uint32_t)total + (uint32_t)(uy(ecu) * W + ux(ecu)) * 79u;
            const uint32_t h = (0u - (mbLo + s)) & 3u;  // head bytes before the first aligned dword
            // bits h + 16 d .. + 15 of the record: the low half of the funnel shift of two of its words
            const uint32_t x = __builtin_amdgcn_alignbit(d < 2 ? w1 : w2, d < 2 ? w0 : w1, h + 16u * (uint32_t)(d & 1));
            const i32x4v v = {(int)expand4(x), (int)expand4(x >> 4), (int)expand4(x >> 8), (int)expand4(x >> 12)};
            __builtin_amdgcn_raw_buffer_store_b128(v, mrs, (int)(s + h) + 16 * d, 0, SC1_MASK ? 16 : 0);
            if (d == 3) {  // bits h + 64 .. h + 75
                typedef int32_t i32x3v __attribute__((ext_vector_type(3)));
                const uint32_t y = w2 >> h;
                const i32x3v t = {(int)expand4(y), (int)expand4(y >> 4), (int)expand4(y >> 8)};
                __builtin_amdgcn_raw_buffer_store_b96(t, mrs, (int)(s + h) + 64, 0, SC1_MASK ? 16 : 0);
            } else {  // byte d of the 3 outside the 19 dwords: head byte d, else tail byte 76 + d
                const bool head = (uint32_t)d < h;
                const uint32_t b = head ? (uint32_t)d : 76u + (uint32_t)d;
                const uint32_t bit = ((head ? w0 : (w2 >> 12)) >> d) & 1u;
                __builtin_amdgcn_raw_buffer_store_b8((char)bit, mrs, (int)(s + b), 0, SC1_MASK ? 16 : 0);
            }
        };
        for (int p0 = 0; p0 < NR; p0 += 16) {
            const bool mine = si >= 0 && (uint32_t)(r - p0) < 16u;
            if (mine) {
                qb[3 * (r - p0)] = cu;
                qb[3 * (r - p0) + 1] = own;
            }
            int k = RI - p0 + incl - n;
            for (uint32_t m = gone; m; m &= m - 1, k++) {
                const uint32_t cz = 32u * (uint32_t)(l & 7) + (uint32_t)__builtin_ctz(m);
                if ((uint32_t)k < 16u) qb[3 * k] = (cz & 15u) | (cz >> 4) << 8 | (uint32_t)((l >> 3) + 1) << 20;
            }
            wsync();
            const bool qa = p0 + q < RI, qr = p0 + q < NR;
            uint32_t qcu = 0, qown = 0, v0 = 0, v1 = 0, v2 = 0;
            if (qr) qcu = qb[3 * q];
            if (qa) {
                qown = qb[3 * q + 1];
                maskBitsDir(T, qcu, (int)(int16_t)qown, d, v0, v1, v2);
            }
            const bool far = qa && ((T.attackFar >> utyp(qcu)) & 1u);
            farAttackRowsDir(far, qcu, d, rows, v0, v1, v2);
            v0 = quadOr(v0);
            v1 = quadOr(v1);
            v2 = quadOr(v2);
            // produce-type bits 23 + ut, when a direction of the quad found a free cell (produce direction bits)
            const uint32_t canProd =
                (uint32_t)(T.prod >> (8 * utyp(qcu))) & 0xFFu & (uplay(qcu) == 0 ? T.aff0 : T.aff1);
            if (((v0 >> (1 + 6 + 12)) & 0xFu) != 0u) v0 |= canProd << (1 + 6 + 16);
            AB_ON(AB_MASKBITS, ablMaskBitsDir(T, qa, far, qcu, qown, d, rows));
            MPHASE(19);
            if (qr && d == 0) {
                const int qc = uy(qcu) * W + ux(qcu), slot = slot0 + uplay(qcu);
                int32_t a[7] = {0, 0, 0, 0, 0, 0, 0};
                if (qa) {
                    const uint64_t lo = (uint64_t)v0 | ((uint64_t)v1 << 32);
                    AB_ON(AB_POLICY, ablSample(slot, lo, v2, qc));
                    uint32_t pk;
                    int picks[3];  // the sampler's type, parameter and produce-type picks
                    sampleBitsRaw(D.pol_seed, polStep, D.pol_slot_base + (uint32_t)slot, NT, K, (lo >> 1) | ((uint64_t)v2 << 63),
                                  (uint64_t)(v2 >> 1), qc, a, &pk, picks);
                    // packFwd(a) for the next launch's decode; the next step of this launch takes the row decoded
                    // here (no cycle lies between the sample and the decode: the unit stands where it stood)
                    if (lastIt) st1<WT_STATE>(st() + stateFwdOff(CAP, HW) + (int)(qown >> 16), (int32_t)pk);
                    qb[3 * q + 2] = sampledDec(qcu, picks[0], picks[1], picks[2]);
                    AB_ON(AB_DECFWD, keepv(sampledDec(launder(qcu), launder(picks[0]), launder(picks[1]), launder(picks[2]))));
                }
                int32_t* dst = D.pol_actions + ((size_t)slot * HW + qc) * 7;
                st4u<WT_MASK>(dst, a[0], a[1], a[2], a[3]);
                st3u<WT_MASK>(dst + 4, a[4], a[5], a[6]);
            }
            MPHASE(13);
            if (qr) {
                AB_SKIP(AB_SKIP_RECORD)
                storeQuad(qcu, v0, v1, v2);
                AB_ON(AB_RECORD, storeQuad(launder(qcu), launder(v0), launder(v1), launder(v2)));
            }
            wsync();
            if (mine) lfwd = qb[3 * (r - p0) + 2];
            wsync();  // read before the next pass lists its entries
        }
        fwdWritten = true;
        MPHASE(14);
    }
    // the fused random policy's action row of cell c of slot (slot0 + i): masked-uniform sample from
    // the parked mask bits (bit k = mask slot k) of an own idle unit, else a zero row
    DEV void policyRow(int slot, int c, int p) const {
        uint64_t lo;
        uint32_t hi;
        cellMaskBits(c, p, lo, hi);
        int32_t a[7];
        if (lo & 1ull) {
            sampleBitsRaw(D.pol_seed, polStep, D.pol_slot_base + (uint32_t)slot, NT, K, (lo >> 1) | ((uint64_t)hi << 63),
                          (uint64_t)(hi >> 1), c, a);
        } else {
#pragma unroll
            for (int q = 0; q < 7; q++) a[q] = 0;
        }
        int32_t* dst = D.pol_actions + ((size_t)slot * HW + c) * 7;
#pragma unroll
        for (int q = 0; q < 7; q++) dst[q] = a[q];
    }
    DEV void writePolicyAll(int slot0, int nslots, int pl0, int pl1) const {
        for (int i = 0; i < nslots; i++)
            for (int c = lid(); c < HW; c += 64) policyRow(slot0 + i, c, i ? pl1 : pl0);
    }
    // rewrite the chunks of the listed dirty cells (rslot[0..n): slot index << 15 | cell)
    DEV void flushDirty(int n, int slot0, int pl0, int pl1) {
        wsync();
        const int total = HW * K;
        const int NCH = (K + 14) / 16 + 1;  // chunks a K-byte record can touch
        for (int base = 0; base < NCH * n; base += 64) {
            const int item = base + lid();
            if (item < NCH * n) {
                const int k = item / NCH, t = item - k * NCH;
                const uint32_t e = rslot[k];
                const int i = (int)(e >> 15), c = (int)(e & 0x7FFFu);
                const int j = ((c * K) >> 4) + t;
                if (j <= ((c * K + K - 1) >> 4))
                    *(uint4*)(D.masks + (size_t)(slot0 + i) * total + 16 * j) = maskChunk(j, i ? pl1 : pl0);
                if (t == 0 && D_HAS(pol_actions) && D_ON(pol_delta)) policyRow(slot0 + i, c, i ? pl1 : pl0);
            }
        }
        wsync();
    }

    // ------------------------------------------------------------------ LightRush
    // ai.abstraction.LightRush with AStarPathFinding, the bot of the reference's LightRush traces
    // (src/tests/GenerateTestTraces.java:84-123), restated for one wave per game.  Generic kernel only, and only
    // in games whose kind names it (k_env: `lr`); the members below are set by lrInit.
    // The bot's memory — AbstractionLayerAI.actions (AbstractionLayerAI.java:36), a LinkedHashMap keyed by Unit —
    // is indexed by unit slot (mrts_internal.h BA_*): an entry's insertion rank orders translateActions'
    // iteration, put() on a live entry keeps its rank, a removed entry that is put again takes a new one.  Java
    // holds Unit references (identity: Unit defines no equals); here a reference is the unit's slot, and
    // lrCompact moves entries and rewrites references when the end-of-step compaction renumbers the slots.  A
    // reference to a removed unit becomes BR_DEAD: Java only ever asks such a unit "are you still in the list"
    // (Attack / Harvest.completed) or compares it with a live unit (LightRush.java:235,246) — both are false.
    // Every scalar below is wave-uniform; the unit scans, the open-list minimum and the bitmaps use the lanes.
    uint32_t* lrMem;    // [2][botPlayerWords(CAP)]: the state block's bot memory (hdr [1] = this step's desires)
    uint32_t* lrKey;    // A*: open key per insertion number
    uint32_t* lrGs;     // positions of gs.getResourceUsage(), bit pos + W (as `bits`)
    uint32_t* lrRu;     // translateActions' running ResourceUsage ru
    uint32_t* lrPa;     // the PlayerAction's ResourceUsage while the desires are composed
    uint32_t* lrFree;   // !gs.free(x, y) per cell
    uint16_t* lrCell;   // A*: cell per insertion number
    uint16_t* lrPar;    // A*: parent cell per cell (0xFFFF = not in open or closed)
    uint16_t* lrCost;   // A*: cost[] per cell (fixed at first discovery: there is no decrease-key)
    uint16_t* lrOrd;    // [2][CAP]: per player the accepted desires' slots in pa order (scratch before that)
    int lrRes0, lrRes1; // resourcesUsed of gs.getResourceUsage()
    DEV void lrInit(uint8_t* q) {
        const int NB2 = (HW + 2 * W + 31) / 32;
        lrMem = (uint32_t*)q; q += 4 * botWords(CAP);
        lrKey = (uint32_t*)q; q += 4 * HW;
        lrGs = (uint32_t*)q; q += 4 * NB2;
        lrRu = (uint32_t*)q; q += 4 * NB2;
        lrPa = (uint32_t*)q; q += 4 * NB2;
        lrFree = (uint32_t*)q; q += 4 * maskWords(HW);
        lrCell = (uint16_t*)q; q += 2 * HW;
        lrPar = (uint16_t*)q; q += 2 * HW;
        lrCost = (uint16_t*)q; q += 2 * HW;
        lrOrd = (uint16_t*)q;
        lrRes0 = lrRes1 = 0;
    }
    DEV uint32_t* lrHdr(int p) const { return lrMem + p * botPlayerWords(CAP); }
    DEV uint32_t* lrArr(int p, int a) const { return lrHdr(p) + BOT_HDR + a * CAP; }
    DEV int lrType(int k) const { return (int)((P.bot_types >> (4 * k)) & 15u); }  // 0 Base 1 Barracks 2 Worker 3 Light
    static DEV uint32_t lrAct(int kind, int ut, int bx, int by) {
        return (uint32_t)kind | ((uint32_t)ut << 4) | (((uint32_t)(bx + 1) & 0xFFu) << 8) | (((uint32_t)by & 0xFFu) << 16);
    }
    static DEV int lrPack(int t, int prm, int ut, int tx, int ty) { return t | (prm & 15) << 4 | ut << 8 | tx << 12 | ty << 20; }
    // the headers and the entries of the slots in use; slots >= nu are empty (this cycle's new units land there)
    DEV void lrLoad() {
        const int32_t* gm = st() + P.bot_off;
        const int PW = botPlayerWords(CAP);
        if (lid() < 2 * BOT_HDR) lrMem[(lid() / BOT_HDR) * PW + lid() % BOT_HDR] = (uint32_t)gm[(lid() / BOT_HDR) * PW + lid() % BOT_HDR];
        for (int p = 0; p < 2; p++) {
            for (int a = 0; a < BA_ARRAYS; a++)
                for (int i = lid(); i < nu; i += 64) lrArr(p, a)[i] = (uint32_t)gm[p * PW + BOT_HDR + a * CAP + i];
            // all three words: lrCompact and lrStore copy a new unit's entry whole, so no LDS leftovers may sit
            // in it (a checkpoint's bytes are a function of the games played)
            for (int a = 0; a < BA_ARRAYS; a++)
                for (int i = nu + lid(); i < CAP; i += 64) lrArr(p, a)[i] = 0u;
        }
        wsync();
    }
    DEV void lrStore() {
        int32_t* gm = st() + P.bot_off;
        const int PW = botPlayerWords(CAP);
        if (lid() < 2 * BOT_HDR) gm[(lid() / BOT_HDR) * PW + lid() % BOT_HDR] = (int32_t)lrMem[(lid() / BOT_HDR) * PW + lid() % BOT_HDR];
        for (int p = 0; p < 2; p++)
            for (int a = 0; a < BA_ARRAYS; a++)
                for (int i = lid(); i < nu; i += 64) gm[p * PW + BOT_HDR + a * CAP + i] = (int32_t)lrArr(p, a)[i];
    }
    DEV void lrClear() {  // AbstractionLayerAI.reset (AbstractionLayerAI.java:53-55) of both sides
        for (int i = lid(); i < botWords(CAP); i += 64) lrMem[i] = 0u;
        wsync();
    }
    // Before compact(): entries follow their units to the compacted slots, entries of removed units go (Java
    // deletes them at the next translateActions, AbstractionLayerAI.java:69-71, and nothing reads them before),
    // references are renumbered.  Units born this cycle sit in slots that held no entry.
    DEV void lrCompact() {
        uint16_t* map = lrOrd;  // old slot -> new slot (free between the issue and the next getAction)
        int base = 0;
        for (int o0 = 0; o0 < nu; o0 += 64) {
            const int o = o0 + lid();
            const bool alive = o < nu && !(uc[o] & UC_DEAD);
            const uint64_t m = ballot(alive);
            if (o < nu) map[o] = alive ? (uint16_t)(base + lanes_below(m)) : (uint16_t)BR_DEAD;
            base += __popcll(m);
        }
        wsync();
        for (int p = 0; p < 2; p++) {
            uint32_t *A = lrArr(p, BA_ACT), *B = lrArr(p, BA_REF), *R = lrArr(p, BA_RANK);
            for (int o0 = 0; o0 < nu; o0 += 64) {
                const int o = o0 + lid();
                const bool alive = o < nu && !(uc[o] & UC_DEAD);
                uint32_t a = 0, b = 0, r = 0;
                if (alive) {
                    a = A[o];
                    b = B[o];
                    r = R[o];
                }
                wsync();
                if (alive) {
                    uint32_t lo = b & 0xFFFFu, hi = b >> 16;
                    if (lo < (uint32_t)nu) lo = map[lo];
                    if (hi < (uint32_t)nu) hi = map[hi];
                    const int idx = map[o];
                    A[idx] = a;
                    B[idx] = lo | (hi << 16);
                    R[idx] = r;
                }
                wsync();
            }
            for (int o = base + lid(); o < nu; o += 64) A[o] = 0u;
        }
        wsync();
    }
    // the first unit in list order at the smallest Manhattan distance from (x, y) (strict `<` in the Java loops):
    // mode 0 an enemy of p (LightRush.java:142-154, Train.java:113-121), 1 a resource (LightRush.java:210-218,
    // Train.java:103-111), 2 a stockpile of p (LightRush.java:220-228).  -1 = none.
    DEV int lrClosest(int x, int y, int p, int mode) const {
        int best = INF;
        for (int o = lid(); o < nu; o += 64) {
            const uint32_t c = uc[o];
            const int pl = uplay(c);
            const uint32_t fl = U.flags[utyp(c)];
            const bool ok = mode == 0 ? (pl >= 0 && pl != p) : mode == 1 ? (fl & F_RESOURCE) != 0 : ((fl & F_STOCKPILE) != 0 && pl == p);
            if (ok && !(c & UC_DEAD)) best = min(best, ((abs(ux(c) - x) + abs(uy(c) - y)) << 16) | o);
        }
        best = wave_min(best);
        return best == INF ? -1 : (best & 0xFFFF);
    }
    DEV int lrCount(int p, int typ, uint32_t flag) const {  // p's units of type typ (flag = 0) or with a type flag
        int n = 0;
        for (int o0 = 0; o0 < nu; o0 += 64) {
            const int o = o0 + lid();
            bool is = false;
            if (o < nu) {
                const uint32_t c = uc[o];
                is = !(c & UC_DEAD) && uplay(c) == p && (flag ? (U.flags[utyp(c)] & flag) != 0 : utyp(c) == typ);
            }
            n += __popcll(ballot(is));
        }
        return n;
    }
    // actions.put(u, aa) (AbstractionLayerAI.java:119-137): a present key keeps its place in the LinkedHashMap
    DEV void lrPut(int p, int s, uint32_t act, uint32_t ref) {
        if (lid() == 0) {
            if ((lrArr(p, BA_ACT)[s] & 7u) == BK_NONE) lrArr(p, BA_RANK)[s] = lrHdr(p)[0]++;
            lrArr(p, BA_ACT)[s] = act;
            lrArr(p, BA_REF)[s] = ref;
        }
        wsync();
    }
    DEV bool lrBit(const uint32_t* b, int i) const { return (uniu(b[i >> 5]) >> (i & 31)) & 1u; }
    DEV void lrSetBit(uint32_t* b, int i) {
        if (lid() == 0) b[i >> 5] |= 1u << (i & 31);
        wsync();
    }
    // gs.getResourceUsage() (rts/GameState.java:652-664) and the cells where gs.free(x, y) is false
    // (rts/GameState.java:191-207: terrain, a unit, or the target of a pending MOVE / PRODUCE).  The other side's
    // parked actions are not assignments yet (both getActions precede either issue), only UA_PRESENT counts.
    DEV void lrGameUsage() {
        const int NB2 = (HW + 2 * W + 31) / 32;
        for (int i = lid(); i < NB2; i += 64) lrGs[i] = 0u;
        for (int i = lid(); i < maskWords(HW); i += 64) lrFree[i] = 0u;
        wsync();
        int s0 = 0, s1 = 0;
        for (int o = lid(); o < nu; o += 64) {
            const uint32_t c = uc[o], a = ua[o];
            const int t = ua_type(a);
            if (!(c & UC_DEAD) && (a & UA_PRESENT) && (t == T_MOVE || t == T_PRODUCE)) {
                const int d = par[o], nx = ux(c) + dxo(d), ny = uy(c) + dyo(d);
                const int pos = ny * W + nx + W;
                atomicOr(&lrGs[pos >> 5], 1u << (pos & 31));
                if (inb(nx, ny)) atomicOr(&lrFree[(ny * W + nx) >> 5], 1u << ((ny * W + nx) & 31));
                if (t == T_PRODUCE) {
                    if (uplay(c) == 0) s0 += U.cost[ua_ut(a)];
                    else s1 += U.cost[ua_ut(a)];
                }
            }
        }
        for (int c = lid(); c < HW; c += 64)
            if (cell[c] != EMPTY) atomicOr(&lrFree[c >> 5], 1u << (c & 31));
        lrRes0 = wave_sum(s0);
        lrRes1 = wave_sum(s1);
        wsync();
    }
    // gs.isUnitActionAllowed(u, ua) (rts/GameState.java:434-457) of a MOVE or PRODUCE in direction d
    DEV bool lrAllowed(int s, int t, int d, int ut) const {
        const uint32_t c = uniu(uc[s]);
        const int nx = ux(c) + dxo(d), ny = uy(c) + dyo(d);
        if (t == T_MOVE && (!inb(nx, ny) || uni(cell[ny * W + nx]) != EMPTY)) return false;
        if (lrBit(lrGs, ny * W + nx + W)) return false;
        const int cost = t == T_PRODUCE ? U.cost[ut] : 0, pl = uplay(c);
        // ResourceUsage.consistentWith (rts/ResourceUsage.java:31-50) with the game's usage as `anotherUsage`
        if (lrRes0 != 0 && lrRes0 + (pl == 0 ? cost : 0) > 0 && lrRes0 + (pl == 0 ? cost : 0) > pres0) return false;
        if (lrRes1 != 0 && lrRes1 + (pl == 1 ? cost : 0) > 0 && lrRes1 + (pl == 1 ? cost : 0) > pres1) return false;
        return true;
    }
    // AStarPathFinding.findPathToPositionInRange (AStarPathFinding.java:52-79) over runAStar
    // (AStarPathFinding.java:175-295): the direction of the first step, or -1 for Java's null (no path, or the
    // start cell already within range).  The Java keeps `open` sorted by descending heuristic + cost, pops from
    // its end and inserts a new element just above the last one whose f is >= its own (addToOpen,
    // AStarPathFinding.java:104-138): the pop is the smallest f, the most recently inserted among equals.  A
    // cell is inserted at most once (inOpenOrClosed), so an insertion number identifies it; the open list here
    // is unsorted — key[n] = f << 12 | (4095 - n), popped = INF — and a pop is the minimum key over the lanes.
    // H * W <= LR_MAX_CELLS: n < 1024, f < 64 + 1024.  (tx, ty) may lie off the map (Build at x = -1): it is
    // only ever compared with, never read.
    DEV int lrAStar(int s, int tx, int ty, int range) {
        MPHASE(27);  // (timing build: 25 behaviours, 26 A*, 27 the rest of translateActions, 28 the issue)
        const int d = lrAStarRun(s, tx, ty, range);
        MPHASE(26);
        return d;
    }
    DEV int lrAStarRun(int s, int tx, int ty, int range) {
        const uint32_t cu = uniu(uc[s]);
        const int sx = ux(cu), sy = uy(cu), start = sy * W + sx;
        for (int c = lid(); c < HW; c += 64) lrPar[c] = 0xFFFFu;
        wsync();
        if (lid() == 0) {
            lrCell[0] = (uint16_t)start;
            lrKey[0] = ((uint32_t)(abs(sx - tx) + abs(sy - ty)) << 12) | 4095u;
            lrPar[start] = (uint16_t)start;
            lrCost[start] = 0;
        }
        wsync();
        int n = 1, goal = -1;
        for (;;) {
            int best = INF;
            for (int i = lid(); i < n; i += 64) best = min(best, (int)lrKey[i]);
            best = wave_min(best);
            if (best == INF) return -1;  // open list empty: no path
            const int idx = 4095 - (best & 4095);
            const int pos = uni(lrCell[idx]);
            const int x = pos % W, y = pos / W;
            if ((x - tx) * (x - tx) + (y - ty) * (y - ty) <= range * range) {
                goal = pos;
                break;
            }
            // the four neighbours in the order up, right, down, left (lanes 0..3): distinct cells, so their
            // tests are independent and their insertion numbers follow the lane order
            const int d = lid();
            bool ok = false;
            int c2 = 0, h2 = 0;
            if (d < 4) {
                const int nx = x + dxo(d), ny = y + dyo(d);
                if (inb(nx, ny)) {
                    c2 = ny * W + nx;
                    h2 = abs(nx - tx) + abs(ny - ty);
                    ok = lrPar[c2] == 0xFFFFu && !((lrFree[c2 >> 5] >> (c2 & 31)) & 1u) &&
                         !((lrRu[(c2 + W) >> 5] >> ((c2 + W) & 31)) & 1u);
                }
            }
            const uint64_t m = ballot(ok);
            const int gc = uni(lrCost[pos]) + 1;
            if (d == 0) lrKey[idx] = (uint32_t)INF;
            if (ok) {
                const int k = n + lanes_below(m);
                lrCost[c2] = (uint16_t)gc;
                lrPar[c2] = (uint16_t)pos;
                lrCell[k] = (uint16_t)c2;
                lrKey[k] = ((uint32_t)(h2 + gc) << 12) | (uint32_t)(4095 - k);
            }
            n += __popcll(m);
            wsync();
        }
        // the first step: walk the parents back from the goal (AStarPathFinding.java:60-78)
        int pos = goal, last = goal;
        for (;;) {
            const int par2 = uni(lrPar[pos]);
            if (par2 == pos) break;
            last = pos;
            pos = par2;
        }
        if (last == pos + W) return 2;
        if (last == pos - 1) return 3;
        if (last == pos - W) return 0;
        if (last == pos + 1) return 1;
        return -1;  // already there
    }
    // Train.score (Train.java:98-127): minus the distance to the closest resource (a harvester) or enemy
    DEV int lrScore(int x, int y, int ut, int p) const {
        const int o = lrClosest(x, y, p, (U.flags[ut] & F_HARVEST) ? 1 : 0);
        if (o < 0) return 0;
        const uint32_t c = uniu(uc[o]);
        return -(abs(ux(c) - x) + abs(uy(c) - y));
    }
    // the direction from (x, y) to the adjacent cell (ax, ay), -1 if it is not adjacent
    static DEV int lrAdjacent(int x, int y, int ax, int ay) {
        int d = -1;
        if (ax == x && ay == y - 1) d = 0;
        if (ax == x + 1 && ay == y) d = 1;
        if (ax == x && ay == y + 1) d = 2;
        if (ax == x - 1 && ay == y) d = 3;
        return d;
    }
    // aa.execute(gs, ru): the UnitAction as lrPack, or -1 for null
    DEV int lrExecute(int p, int s, uint32_t act, uint32_t ref) {
        const uint32_t cu = uniu(uc[s]);
        const int x = ux(cu), y = uy(cu), typ = utyp(cu);
        const int kind = (int)(act & 7u), ut = (int)((act >> 4) & 15u);
        if (kind == BK_TRAIN) {  // Train.execute (Train.java:48-96)
            int bestD = -1, bestS = -1;
            for (int d = 0; d < 4; d++) {
                const int nx = x + dxo(d), ny = y + dyo(d);
                if (!inb(nx, ny) || lrBit(lrFree, ny * W + nx)) continue;
                const int sc = lrScore(nx, ny, ut, p);
                if (sc > bestS || bestD == -1) {
                    bestS = sc;
                    bestD = d;
                }
            }
            if (lid() == 0) lrArr(p, BA_ACT)[s] = act | 8u;  // completed = true, action or not
            wsync();
            if (bestD != -1 && lrAllowed(s, T_PRODUCE, bestD, ut)) return lrPack(T_PRODUCE, bestD, ut, 0, 0);
            return -1;
        }
        if (kind == BK_BUILD) {  // Build.execute (Build.java:54-78)
            const int bx = (int)((act >> 8) & 0xFFu) - 1, by = (int)((act >> 16) & 0xFFu);
            const int mv = lrAStar(s, bx, by, 1);
            if (mv >= 0) return lrAllowed(s, T_MOVE, mv, 0) ? lrPack(T_MOVE, mv, 0, 0, 0) : -1;
            const int d = lrAdjacent(x, y, bx, by);
            if (d >= 0 && lrAllowed(s, T_PRODUCE, d, ut)) return lrPack(T_PRODUCE, d, ut, 0, 0);
            return -1;
        }
        if (kind == BK_HARVEST) {  // Harvest.execute (Harvest.java:72-114)
            const bool carrying = uni(res[s]) != 0;
            const uint32_t r = carrying ? (ref >> 16) : (ref & 0xFFFFu);
            if (r >= BR_DEAD) return -1;  // target / base == null
            const uint32_t tc = uniu(uc[r]);
            const int mv = lrAStar(s, ux(tc), uy(tc), 1);
            if (mv >= 0) return lrAllowed(s, T_MOVE, mv, 0) ? lrPack(T_MOVE, mv, 0, 0, 0) : -1;
            const int d = lrAdjacent(x, y, ux(tc), uy(tc));
            return d >= 0 ? lrPack(carrying ? T_RETURN : T_HARVEST, d, 0, 0, 0) : -1;
        }
        if (kind == BK_ATTACK) {  // Attack.execute (Attack.java:51-65)
            const uint32_t r = ref & 0xFFFFu;
            if (r >= BR_DEAD) return -1;
            const uint32_t tc = uniu(uc[r]);
            const int dx = ux(tc) - x, dy = uy(tc) - y, rg = U.range[typ];
            // Math.sqrt(dx * dx + dy * dy) <= attackRange: the integer test (sqrt is monotone, sqrt(r * r) = r exactly)
            if (dx * dx + dy * dy <= rg * rg) return lrPack(T_ATTACK, -1, 0, ux(tc), uy(tc));
            const int mv = lrAStar(s, ux(tc), uy(tc), rg);
            return (mv >= 0 && lrAllowed(s, T_MOVE, mv, 0)) ? lrPack(T_MOVE, mv, 0, 0, 0) : -1;
        }
        return -1;
    }
    // aa.completed(gs): Train.java:29-31, Build.java:33-37, Harvest.java:42-48, Attack.java:30-33
    DEV bool lrCompleted(int s, uint32_t act, uint32_t ref) const {
        switch (act & 7u) {
            case BK_TRAIN: return (act & 8u) != 0;
            case BK_BUILD: {
                const int bx = (int)((act >> 8) & 0xFFu) - 1, by = (int)((act >> 16) & 0xFFu);
                return inb(bx, by) && uni(cell[by * W + bx]) < CAP;  // getUnitAt(x, y) != null
            }
            case BK_HARVEST: return (uni(res[s]) > 0 ? (ref >> 16) : (ref & 0xFFFFu)) >= BR_DEAD;
            case BK_ATTACK: return (ref & 0xFFFFu) >= BR_DEAD;
        }
        return true;
    }
    // AbstractionLayerAI.findBuildingPosition (AbstractionLayerAI.java:143-229): rings l = 1.., sides up, right,
    // down, left, on pgs.getAllFree() (rts/PhysicalGameState.java:512-525: terrain and units only), skipping
    // the reserved positions; -1 when nothing is free.  Serial on purpose (one uniform LDS read per candidate cell):
    // it runs only when a Build is newly placed — at most twice per getAction, a handful of times per game — and
    // the first ring almost always holds a free cell; the order of the scan is the result, so lanes would have to
    // ballot per ring side to keep it.  Worst case (a full map) is about 4 * max(H, W)^2 reads.
    DEV int lrBuildingPosition(int r0, int r1, int dx0, int dy0) const {
        const int L = max(H, W);
        for (int l = 1; l < L; l++)
            for (int side = 0; side < 4; side++) {
                const bool horiz = !(side & 1);
                const int fixed = side == 0 ? dy0 - l : side == 1 ? dx0 + l : side == 2 ? dy0 + l : dx0 - l;
                if (fixed < 0 || fixed >= (horiz ? H : W)) continue;
                for (int k = -l; k <= l; k++) {
                    const int x = horiz ? dx0 + k : fixed, y = horiz ? fixed : dy0 + k;
                    if (!inb(x, y)) continue;
                    const int pos = x + y * W;
                    if (pos != r0 && pos != r1 && uni(cell[pos]) == EMPTY) return pos;
                }
            }
        return -1;
    }
    // AbstractionLayerAI.buildIfNotAlreadyBuilding (AbstractionLayerAI.java:231-245): only the held action's class
    // and type are compared.  build(u, type, pos % W, pos / W) with Java's % and / : -1 gives x = -1, y = 0.
    DEV void lrBuild(int p, int s, int ut, int& r0, int& r1) {
        const uint32_t act = uniu(lrArr(p, BA_ACT)[s]);
        if ((act & 7u) == BK_BUILD && (int)((act >> 4) & 15u) == ut) return;
        const uint32_t cu = uniu(uc[s]);
        const int pos = lrBuildingPosition(r0, r1, ux(cu), uy(cu));
        lrPut(p, s, lrAct(BK_BUILD, ut, pos < 0 ? -1 : pos % W, pos < 0 ? 0 : pos / W), BR_NULL | (BR_NULL << 16));
        if (r0 == -2) r0 = pos;
        else r1 = pos;
    }
    // LightRush.meleeUnitBehavior (LightRush.java:142-159)
    DEV void lrMelee(int p, int s) {
        const uint32_t cu = uniu(uc[s]);
        const int e = lrClosest(ux(cu), uy(cu), p, 0);
        if (e >= 0) lrPut(p, s, lrAct(BK_ATTACK, 0, -1, 0), (uint32_t)e | (BR_NULL << 16));
    }
    // LightRush.getAction (LightRush.java:77-121) of player p: the parked actions (UA_PA) and their order (lrOrd,
    // hdr [1]) are the PlayerAction before its fillWithNones; lrIssue issues it.
    DEV void lightRush(int p) {
        const int tBase = lrType(0), tBarracks = lrType(1), tWorker = lrType(2), tLight = lrType(3);
        const int have = pres(p);
        MPHASE(2);
        lrGameUsage();
        // bases, barracks, melee units: idle ones, in list order (LightRush.java:83-107)
        const bool trainWorker = lrCount(p, tWorker, 0) < 1 && have >= U.cost[tWorker];  // baseBehavior (LightRush.java:123-134)
        const bool trainLight = have >= U.cost[tLight];                                  // barracksBehavior (LightRush.java:136-140)
        for (int pass = 0; pass < 3; pass++)
            for (int o0 = 0; o0 < nu; o0 += 64) {
                const int o = o0 + lid();
                bool is = false;
                if (o < nu) {
                    const uint32_t c = uc[o];
                    const uint32_t fl = U.flags[utyp(c)];
                    is = !(c & UC_DEAD) && uplay(c) == p && !(ua[o] & UA_PRESENT) &&
                         (pass == 0 ? utyp(c) == tBase : pass == 1 ? utyp(c) == tBarracks : ((fl & F_ATTACK) && !(fl & F_HARVEST)));
                }
                for (uint64_t m = ballot(is); m; m &= m - 1) {
                    const int s = o0 + __builtin_ctzll(m);
                    if (pass == 0) {
                        if (trainWorker) lrPut(p, s, lrAct(BK_TRAIN, tWorker, -1, 0), BR_NULL | (BR_NULL << 16));
                    } else if (pass == 1) {
                        if (trainLight) lrPut(p, s, lrAct(BK_TRAIN, tLight, -1, 0), BR_NULL | (BR_NULL << 16));
                    } else {
                        lrMelee(p, s);
                    }
                }
            }
        // workersBehavior (LightRush.java:161-258) over every worker of p, idle or not
        const int nWorkers = lrCount(p, 0, F_HARVEST);
        if (nWorkers > 0) {
            int used = 0, wBase = -1, wBarracks = -1;  // the worker-list index that builds a base / a barracks
            if (lrCount(p, tBase, 0) == 0 && have >= U.cost[tBase] + used) {
                wBase = 0;
                used += U.cost[tBase];
            }
            if (lrCount(p, tBarracks, 0) == 0 && have >= U.cost[tBarracks] + used && nWorkers > wBase + 1) {
                wBarracks = wBase + 1;
                used += U.cost[tBarracks];
            }
            int r0 = -2, r1 = -2, wi = 0, nFree = 0;  // reservedPositions; stillFreeWorkers go to lrOrd
            uint16_t* stillFree = lrOrd + p * CAP;
            for (int o0 = 0; o0 < nu; o0 += 64) {
                const int o = o0 + lid();
                bool is = false;
                if (o < nu) {
                    const uint32_t c = uc[o];
                    is = !(c & UC_DEAD) && uplay(c) == p && (U.flags[utyp(c)] & F_HARVEST);
                }
                for (uint64_t m = ballot(is); m; m &= m - 1, wi++) {
                    const int s = o0 + __builtin_ctzll(m);
                    if (wi == wBase) {
                        lrBuild(p, s, tBase, r0, r1);
                        continue;
                    }
                    if (wi == wBarracks) {
                        lrBuild(p, s, tBarracks, r0, r1);
                        continue;
                    }
                    const uint32_t cu = uniu(uc[s]);
                    const int rsrc = lrClosest(ux(cu), uy(cu), p, 1), home = lrClosest(ux(cu), uy(cu), p, 2);
                    const uint32_t act = uniu(lrArr(p, BA_ACT)[s]), ref = uniu(lrArr(p, BA_REF)[s]);
                    const bool isH = (act & 7u) == BK_HARVEST;
                    bool free = true;
                    if (uni(res[s]) > 0) {
                        if (home >= 0) {  // harvest(u, null, closestBase) unless it already returns to that base
                            if (!isH || (ref >> 16) != (uint32_t)home)
                                lrPut(p, s, lrAct(BK_HARVEST, 0, -1, 0), BR_NULL | ((uint32_t)home << 16));
                            free = false;
                        }
                    } else if (rsrc >= 0 && home >= 0) {
                        if (!isH || (ref & 0xFFFFu) != (uint32_t)rsrc || (ref >> 16) != (uint32_t)home)
                            lrPut(p, s, lrAct(BK_HARVEST, 0, -1, 0), (uint32_t)rsrc | ((uint32_t)home << 16));
                        free = false;
                    }
                    if (free) {
                        if (lid() == 0) stillFree[nFree] = (uint16_t)s;
                        nFree++;
                    }
                }
            }
            wsync();
            for (int i = 0; i < nFree; i++) lrMelee(p, uni(stillFree[i]));
        }
        MPHASE(25);
        lrTranslate(p);
        MPHASE(27);
    }
    // AbstractionLayerAI.translateActions (AbstractionLayerAI.java:58-113)
    DEV void lrTranslate(int p) {
        const int NB2 = (HW + 2 * W + 31) / 32;
        uint32_t *A = lrArr(p, BA_ACT), *B = lrArr(p, BA_REF), *R = lrArr(p, BA_RANK);
        uint16_t* ord = lrOrd + p * CAP;
        for (int i = lid(); i < NB2; i += 64) {
            lrRu[i] = 0u;
            lrPa[i] = lrGs[i];
        }
        wsync();
        int nd = 0, last = -1;
        for (;;) {  // the entries in insertion order
            int best = INF;
            for (int s = lid(); s < nu; s += 64)
                if ((A[s] & 7u) != BK_NONE && (int)R[s] > last) best = min(best, (int)R[s]);
            best = wave_min(best);
            if (best == INF) break;
            int sl = INF;
            for (int s = lid(); s < nu; s += 64)
                if ((A[s] & 7u) != BK_NONE && (int)R[s] == best) sl = s;
            sl = wave_min(sl);
            last = best;
            const uint32_t act = uniu(A[sl]), ref = uniu(B[sl]);
            if (lrCompleted(sl, act, ref)) {  // toDelete (removal after the loop: nothing in it reads the map)
                if (lid() == 0) A[sl] = BK_NONE;
                wsync();
                continue;
            }
            if (uniu(ua[sl]) & UA_PRESENT) continue;
            const int r = lrExecute(p, sl, act, ref);
            if (r < 0) continue;
            const int t = r & 15, prm = (r >> 4) & 15;
            if (lid() == 0) {  // the desire, parked without UA_PA until it is accepted
                ua[sl] = pack_ua(t, (r >> 8) & 15, (r >> 12) & 0xFF, (r >> 20) & 0xFF);
                par[sl] = (int16_t)(t == T_ATTACK ? -1 : prm);
                ord[nd] = (uint16_t)sl;
            }
            nd++;
            wsync();
            if (t == T_MOVE || t == T_PRODUCE) {  // ru.merge(ua.resourceUsage(...)): A* treats these cells as blocked
                const uint32_t cu = uniu(uc[sl]);
                lrSetBit(lrRu, (uy(cu) + dyo(prm)) * W + ux(cu) + dxo(prm) + W);
            }
        }
        // the desires consistent with gs.getResourceUsage() and the ones accepted before them
        // (AbstractionLayerAI.java:101-109, ResourceUsage.consistentWith with the desire as `anotherUsage`)
        int run = p == 0 ? lrRes0 : lrRes1, na = 0;
        for (int i = 0; i < nd; i++) {
            const int sl = uni(ord[i]);
            const uint32_t a = uniu(ua[sl]), cu = uniu(uc[sl]);
            const int t = ua_type(a), prm = uni(par[sl]);
            const bool mp = t == T_MOVE || t == T_PRODUCE;
            const int pos = (uy(cu) + dyo(prm)) * W + ux(cu) + dxo(prm) + W;
            const int cost = t == T_PRODUCE ? U.cost[ua_ut(a)] : 0;
            bool ok = !(mp && lrBit(lrPa, pos));
            if (cost != 0 && run + cost > 0 && run + cost > pres(p)) ok = false;
            if (!ok) continue;
            if (lid() == 0) {
                ua[sl] = a | UA_PA;
                ord[na] = (uint16_t)sl;
            }
            if (mp) lrSetBit(lrPa, pos);
            run += cost;
            na++;
            wsync();
        }
        if (lid() == 0) lrHdr(p)[1] = (uint32_t)na;
        wsync();
    }
    // issueSafe of the PlayerAction: the accepted desires in their order, then fillWithNones(gs, p, 10) in list
    // order (AbstractionLayerAI.java:111)
    DEV void lrIssue(int p) {
        MPHASE(3);
        curP = p;
        const int n = (int)uniu(lrHdr(p)[1]);
        for (int b = 0; b < n; b += 64) {
            const int i = b + lid();
            const bool act = i < n;
            issuePA(act ? (int)lrOrd[p * CAP + i] : 0, act, lid(), min(64, n - b));
        }
        issueFills(p, 10);
        MPHASE(28);
    }

#ifdef MRTS_ABLATE
    // ------------------------------------------------------------------ the ablation build's second copies
    // What a site's AB_ON line runs where the copy is longer than the line: each takes what its site passes, launders
    // it so that the copy cannot be merged with the original, and says why running it leaves the game as it was.
    // selfPlayFast -----
    // AB_DECFWD: the forwarded row's decode once more — the unpack of the decoded word (dec: the steady instance from
    // a launch's second step on) or decodeFwd; nothing written
    DEV void ablDecFwd(bool idle, bool dec, uint32_t cu) {
        if (!(idle && fwdOn)) return;
        if (dec) {
            const uint32_t w = launder(lfwd);
            keepv(ua_type(w) + ua_ut(w) + ua_tx(w) + ua_ty(w) + ((int)(w >> 24) - 1) + (int)(w & 0xFFFFFFu));
        } else {
            int t2 = 0, pr2 = -1, ut2 = 0, tx2 = 0, ty2 = 0;
            const bool bad2 = decodeFwd(launder(cu), launder(lfwd), t2, pr2, ut2, tx2, ty2);
            keepv((int)pack_ua(t2, ut2, tx2, ty2) + pr2 + (int)bad2);
        }
    }
    // AB_ISSUE: the merged pass once more: the test (scratch only), then the writes (idempotent: the same words to the
    // same places; the sequence number and the issue index's sums put back)
    DEV void ablIssueBoth(bool act, bool bad, uint32_t cu, uint32_t adec, int pr) {
        int q0, q1, d0, d1;
        keepv((int)issueBothTest(act, launder(cu), launder(adec), launder(pr), q0, q1, d0, d1));
        const int seqS = seq, sp0 = sumProd0, sp1 = sumProd1, mp0 = maxProd0, mp1 = maxProd1;
        const bool amp = anyMP;
        issueBothWrite(act, bad, launder(cu), launder(adec), launder(pr), q0, q1, d0, d1);
        seq = seqS, sumProd0 = sp0, sumProd1 = sp1, maxProd0 = mp0, maxProd1 = mp1, anyMP = amp;
    }
    // AB_ACCEPT: the acceptance chain once more on copies of the running sums (nothing written)
    DEV void ablAccept(int p, int run0, int run1, bool cand, int rank, int ncand, int t, int pr, int c, uint32_t adec) {
        int r0 = run0, r1 = run1, ir = 0;
        const uint64_t a2 = acceptChain(p, r0, r1, cand, launder(rank), ncand, launder(t), launder(pr), launder(c),
                                        launder(adec), true, ir);
        keepv(ir + (int)a2 + r0 + r1);
    }
    // AB_LEGAL: issueSafe's legality test once more on copies of the row (it rewrites only its arguments)
    DEV void ablLegal(int l, uint32_t cu, int t, int pr, int tx, int ty, int ut) {
        int a1 = launder(t), a2 = launder(pr), a3 = launder(tx), a4 = launder(ty), a5 = launder(ut);
        legality(l, launder(cu), a1, a2, a3, a4, a5);
        keepv(a1 + a2 + a3 + a4 + a5);
    }
    // cycleLanes -----
    // AB_CYCLERANK: the ready test and the rank by sequence number once more (nothing written)
    DEV void ablCycleRank(int l, uint32_t a, uint32_t cu, int prm, int sq) {
        bool rd = false;
        const uint32_t a2 = launder(a), c2 = launder(cu);
        const int p2 = launder(prm), q2 = launder(sq);
        if (l < nu && (a2 & UA_PRESENT))
            rd = etaFlat(ua_type(a2), p2, ua_ut(a2), utyp(c2)) + launder(at[l]) <= time;
        int rk = 0;
        for (uint64_t m = ballot(rd && ua_type(a2) != T_NONE); m; m &= m - 1) rk += rl(q2, __builtin_ctzll(m)) < q2;
        keepv(rk);
    }
    // AB_MOVEBATCH: the lane-parallel MOVE pass once more (the same cells and words written again; no second collision
    // test)
    DEV void ablMoveBatch(bool mv, uint32_t cu, int prm, int target) {
        wsync();
        if (mv) cell[launder(uy(cu) * W + ux(cu))] = EMPTY;
        moveBatch(mv, launder(cu), launder(prm), launder(target), false);
    }
    // AB_EXECLOOP: the execute loop without its executes (they are not idempotent): each ready item's pick and lane
    // reads (nothing written)
    DEV void ablExecLoop(bool wk, int rank, int nw, uint32_t cu, uint32_t a, int prm) {
        const int rk2 = launder(rank);
        for (int r = 0; r < nw; r++) {
            const int k = __builtin_ctzll(ballot(wk && rk2 == r));
            uint32_t c = uniu((uint32_t)rl((int)cu, k));
            if ((launder(killedLanes) >> k) & 1ull) c |= UC_DEAD;
            keepv(c + (uniu((uint32_t)rl((int)a, k)) & ~(UA_READY | UA_PRESENT)) + (uint32_t)rl(prm, k) + (uint32_t)k);
        }
    }
    // the PO renderers -----
    // AB_COUNT: the render-item counters (contended global atomics: only when counting)
    DEV void ablCountRender(int l, int n, uint32_t delta) {
        if (l != 0) return;
        atomicAdd(&g_dbg[0], (unsigned long long)n);
        atomicAdd(&g_dbg[1], 1ull);
        if (delta) atomicAdd(&g_dbg[2], 1ull);
    }
    // AB_PO_ZEROSTORE: a rendered chunk's values kept alive in place of their stores
    DEV void ablKeepChunk(const int (&vv)[4][8]) {
        int acc = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) acc += vv[0][k] ^ vv[1][k] ^ vv[2][k] ^ vv[3][k];
        keepv(acc);
    }
    // writeMasksLanes / writeMasksSteady -----
    // AB_MASKSETUP: the set-up once more: the same bitmaps cleared and filled again (two: a second slot, pl1's)
    DEV void ablMaskSetup(uint32_t* nb, int NW, int MW, uint32_t* rows, bool rowB, bool two, int pl0, int pl1) {
        const int l = lid();
        wsync();
        if (l < NW) nb[l] = 0;
        if (rowB && l < 2 * H) rows[l] = 0;
        int si2 = -1;
        uint32_t cu2 = 0;
        if (l < nu) {
            cu2 = launder(uc[l]);
            if (!(cu2 & UC_DEAD) && !(launder(ua[l]) & UA_PRESENT)) {
                const int op = uplay(cu2);
                if (op >= 0 && op == pl0) si2 = 0;
                else if (two && op >= 0 && op == pl1) si2 = 1;
            }
        }
        const int c2 = uy(cu2) * W + ux(cu2);
        wsync();
        if (si2 >= 0) atomicOr(&nb[si2 * MW + (c2 >> 5)], 1u << (c2 & 31));
        if (rowB && l < nu && !(cu2 & UC_DEAD) && uplay(cu2) >= 0) atomicOr(&rows[uplay(cu2) * H + uy(cu2)], 1u << ux(cu2));
    }
    // AB_TABLES: maskTables once more (a read of the unit-type table and the players' resources)
    DEV void ablTables() {
        const MaskTables T2 = maskTables();
        keepv(T2.attack1 ^ T2.attackFar ^ T2.harvest ^ T2.move ^ T2.resource ^ T2.stockpile ^ T2.aff0 ^ T2.aff1 ^
              (uint32_t)T2.prod);
    }
    // AB_MASKBITS, writeMasksLanes: a second copy of whichever form ran (qb: the quads' scratch, which the copy fills
    // with the same words; else registers only)
    DEV void ablMaskBits(const MaskTables& T, int si, uint32_t cu, int carried, uint32_t* rows, uint32_t* qb) {
        uint32_t v0 = 0, v1 = 0, v2 = 0;
        const uint32_t cu2 = launder(cu);
        if (qb) {
            wsync();
            maskBitsQuads(T, launder(si), cu2, launder(carried), rows, v0, v1, v2, qb);
        } else {
            if (si >= 0) maskBitsFast(T, cu2, launder(carried), v0, v1, v2);
            farAttackRows(si >= 0 && ((T.attackFar >> utyp(cu2)) & 1u), cu2, rows, v0, v1, v2);
        }
        keepv(v0 ^ v1 ^ v2);
    }
    // AB_MASKBITS, writeMasksSteady: the quad's bits once more (registers only)
    DEV void ablMaskBitsDir(const MaskTables& T, bool qa, bool far, uint32_t qcu, uint32_t qown, int d, uint32_t* rows) {
        uint32_t u0 = 0, u1 = 0, u2 = 0;
        const uint32_t qcu2 = launder(qcu);
        if (qa) maskBitsDir(T, qcu2, (int)(int16_t)launder(qown), d, u0, u1, u2);
        farAttackRowsDir(far, qcu2, d, rows, u0, u1, u2);
        keepv(quadOr(u0) ^ quadOr(u1) ^ quadOr(u2));
    }
    // AB_POLICY: the row sampled once more into a scratch row (a pure function of seed, step, slot, cell and bits)
    DEV void ablSample(int slot, uint64_t lo, uint32_t w2, int c) {
        int32_t a2[7];
        sampleBitsRaw(D.pol_seed, polStep, D.pol_slot_base + (uint32_t)launder(slot), NT, K,
                      launder((lo >> 1) | ((uint64_t)w2 << 63)), launder((uint64_t)(w2 >> 1)), launder(c), a2);
        keepv(a2[0] + a2[1] + a2[2] + a2[3] + a2[4] + a2[5] + a2[6]);
    }
    // k_env's step loop -----
    // AB_NEXTSTEP: nextStep once more, from the same flags; the step counters put back
    DEV void ablNextStep() {
        const bool fw = fwdWritten, pl = poLds;
        nextStep();
        fwdWritten = fw;
        poLds = pl;
        polStep--;
        uniStep--;
    }
    // AB_PRIO: the idle count and the SIMD rank once more on a copy of the rank's state (the same entry posted twice);
    // rankC, left: the estimate's constant and the steps left (simdRankStep)
    template <class Rank>
    DEV void ablPrio(const Rank& srank, int rankC, int left) {
        const int wq2 = nu + (int)__popcll(ballot(lid() < nu && !(launder(lua) & UA_PRESENT) && uplay(launder(lcu)) >= 0));
        Rank s2 = srank;
        s2.seen = launder(s2.seen);
        keepv(simdRankStep(s2, (uint32_t)(wq2 + rankC) * (uint32_t)left) + (int)s2.seen);
    }
    // AB_REWARD (the steady instance): the full write of the reward / done pair once more, whether or not the step's
    // own store ran (the same values)
    DEV void ablRewardStores(int slot0, bool gameover, int winner, bool reset) {
        if (lane_id() < 2) {
            D.reward[slot0 + lane_id()] = gameover ? (winner == lane_id() ? 1.0 : -1.0) : 0.0;
            D.done[slot0 + lane_id()] = reset ? 1 : 0;
        }
    }
#endif
#undef D
};

// PassiveAI.getAction = fillWithNones(gs, p, 10) (ai/PassiveAI.java:41-45): nothing to park, the
// list-order fill in issuePlayer does it; RandomBiasedAI and LightRush park their actions.
// LR: the instance can hold a LightRush game (the generic step kernel).
template <bool LR = false, class GameT>
DEV void aiGetAction(GameT& G, int kind, int p) {
    if (kind == GK_RANDOM_BIASED) G.randomBiased(p);
    if (LR && MRTS_UNLIKELY(kind == GK_LIGHT_RUSH)) G.lightRush(p);
}
// The in-step auto-reset's terrain: PhysicalGameState.load(mapPath) runs on every reset
// (JNIGridnetClientSelfPlay.java:221-247, JNIGridnetClient.java:235-258), so the map's own walls come back even where
// mrts_set_state_json had brought others.  From the template's terrain words `tt`: the walls of the LDS cell map (the
// template's units, already placed, stand on none), the state block's terrain words `bt`, which the next launch loads,
// and the terrain plane of the game's `nslots` observations (`obs5`, or null), which a multi-step launch stores with its
// first observation write only.  Out of line: the path is rare, and inlined it took registers from the step loop.
__attribute__((noinline)) static __device__ void restoreMapTerrain(uint16_t* cell, const int32_t* tt, int32_t* bt, int32_t* obs5,
                                                                   int nslots, int slotWords, int HW, int lane) {
    for (int w = lane; w < (HW + 3) / 4; w += 64) {
        const uint32_t v = (uint32_t)tt[w];
        bt[w] = (int32_t)v;
        for (int b = 0; b < 4; b++) {
            const int c = 4 * w + b;
            if (c >= HW) break;
            const bool wall = ((v >> (8 * b)) & 0xFFu) != 0;
            if (wall) cell[c] = WALL;
            else if (cell[c] == WALL) cell[c] = EMPTY;
            if (obs5)
                for (int i = 0; i < nslots; i++) obs5[(size_t)i * slotWords + c] = wall ? 1 : 0;
        }
    }
}

template <bool LR = false, class GameT>
DEV void aiIssue(GameT& G, int kind, int p) {
    if (LR && MRTS_UNLIKELY(kind == GK_LIGHT_RUSH)) G.lrIssue(p);
    else G.issuePlayer(p, 10, true);
}

// Specialisations (FIX = map width, square maps): batches of self-play games with grid actions and a
// built-in unit-type table (K = 79, 7 types, attack window 7), the map size, unit slots FCAP and
// observability compile-time constants, so LDS offsets fold into immediates and the bot / Java-row
// code vanishes — c3 (16x16, 320 slots), c2 (8x8, 128), c5 (32x32 PO, 320 slots = max_units 256).
// FIX = 0: anything (launchEnv picks).
// The helper wave of a HELP launch (8x8 fused uniform multi-step rollouts, BASELINE c2: one game per
// SIMD, so the SIMD idles while the game's wave runs its dependent chain).  Work with no input from the
// game's state moves to a second wave of the workgroup: the unmasked uniform rows (a pure function of
// slot, step and cell) of the NEXT step — to the action tensor, and packed into LDS for the game wave's
// decode — and the observation planes of the PREVIOUS step from the cells the game wave packed.  One
// workgroup barrier per step (A_k: rows(k) ready, obs cells of step k - 1 packed); each LDS buffer is
// double-buffered by step parity, so a buffer is rewritten only after the other wave passed the
// barrier that ends its use.  Output: every buffer ends exactly as after the same steps in one wave.
DEV void helperLoop(const KDyn& D, uint8_t* smem, int g, int niter) {
    constexpr int HW = 64, NT = 7, K = 79;
    const int l = (int)threadIdx.x - 64;
    uint32_t* rowbuf = (uint32_t*)(smem + D.help_off);  // [parity][player slot][cell]
    uint32_t* obsbuf = rowbuf + 2 * 2 * HW;             // [parity][cell][2]
    const int slot0 = 2 * g;
    auto rowsOf = [&](int k) {
        for (int i = 0; i < 2; i++) {
            int32_t a[7];
            uniformRow(D.uni_seed, D.uni_step + (uint32_t)k, D.uni_slot_base + (uint32_t)(slot0 + i), l, NT, K - 23 - NT, a);
            int32_t* dst = D.uni_actions + ((size_t)(slot0 + i) * HW + l) * 7;
            st4u<false>(dst, a[0], a[1], a[2], a[3]);
            st3u<false>(dst + 4, a[4], a[5], a[6]);
            rowbuf[(k & 1) * 2 * HW + i * HW + l] = packFwd(a);
        }
    };
    auto render = [&](int k) {
        if (!D.obs) return;
        const uint32_t w0 = obsbuf[(k & 1) * 2 * HW + 2 * l], w1 = obsbuf[(k & 1) * 2 * HW + 2 * l + 1];
        int v[6];
        v[0] = (int)(int16_t)(w0 & 0xFFFFu);
        v[1] = (int)(int16_t)(w0 >> 16);  // resources, signed as writeObsFull stores them
        v[3] = (int)((w1 >> 4) & 15u);
        v[4] = (int)((w1 >> 8) & 15u);
        v[5] = (int)((w1 >> 12) & 1u);
        const int own = (int)(w1 & 15u);  // player + 1, 0 = none
        int32_t* o0 = D.obs + (size_t)slot0 * D.C * HW;
        const __amdgpu_buffer_rsrc_t rs = bufRsrc(o0, (uint32_t)(2 * D.C * HW * 4));
        // the static terrain plane: first write of the launch, and the step of an auto-reset (packObs' bit 13: the map's
        // own walls are back, restoreMapTerrain)
        const int npl = (k == 0 || ((w1 >> 13) & 1u)) ? 6 : 5;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            v[2] = own ? ((own - 1 + i) % 2) + 1 : 0;  // ((owner + player) % 2) + 1 (GameState.java:947-949)
#pragma unroll
            for (int q = 0; q < 6; q++) {
                if (q >= npl) break;
                const uint32_t off = (uint32_t)((i * D.C + q) * HW + l);
                __builtin_amdgcn_raw_buffer_store_b32(v[q], rs, (int)(off * 4u), 0, 16);
            }
            if (MRTS_UNLIKELY(D.obs16 != nullptr)) {
                int16_t* h0 = D.obs16 + (size_t)(slot0 + i) * D.C * HW;
#pragma unroll
                for (int q = 0; q < 6; q++) h0[(size_t)q * HW + l] = (int16_t)v[q];
            }
            if (MRTS_UNLIKELY(D.obs8 != nullptr)) {  // the uint8 transport: every plane, every step
                uint8_t* b0 = D.obs8 + (size_t)(slot0 + i) * D.C * HW;
#pragma unroll
                for (int q = 0; q < 6; q++) b0[(size_t)q * HW + l] = (uint8_t)v[q];
            }
        }
    };
    rowsOf(0);
    __syncthreads();  // A_0
    for (int k = 0; k < niter; k++) {
        if (k + 1 < niter) rowsOf(k + 1);
        __syncthreads();  // A_{k+1}: the game wave packed step k's cells; rows(k + 1) are in LDS
        render(k);
    }
}

// Issue priority by rank among the waves that share a SIMD (multi-step launches, KDyn.prio_tab).  A
// launch ends with its slowest SIMD, and a SIMD with its last game: the four games of a SIMD finish
// far apart (round 3 span build: 1.6-2.9 ms in a 200-step c3 launch), while the heaviest game alone
// needs ~2.2 ms and the SIMD's whole issue work ~2.0 ms.  So the game with the most remaining work
// (longest processing time first) should issue first, the next one second, and so on — a ranking
// the absolute unit-count thresholds only approximate.  Each wave posts, once per step, its game's
// remaining-work estimate (units + own idle units, times the steps left in the launch) with the
// launch stamp into its SIMD's row of the table (key from HW_ID / XCC_ID, slot = wave id), reads the
// row back, and at its next step sets s_setprio 3 - rank.  The reads may be a step old or see a
// neighbour's entry mid-update: priority never changes what a game computes, only when it issues.
// The estimate is (units + own idle units + RANK_C) x steps left.  One game alone on a SIMD takes ~ a + b x units
// per step with a / b ~ 75 units (E = 1024 span data), so the steps left dominate: the games that fell behind issue
// first (c3, 3 runs each: C = 0 315.5 / 285.3 M at K = 200 / 20, C = 75 334.4 / 285.5, C = 150 334.1 / 280.7, C = 400
// 333.6 / 284.5; later, with balanced placement and the byte image, C = 4000 vs 400: K = 20 kernel 11.95 vs 12.08 us
// per step over 4 pairs, K = 200 equal — a game one step behind always outranks, units break ties).
constexpr int RANK_C = 4000;
struct SimdRank {
    uint32_t* row;  // this SIMD's 16 entries (stamp << 24 | estimate; 0 = free)
    int me;         // this wave's slot in the row
    uint32_t tag;   // this launch's stamp byte, never 0
    uint32_t seen;  // lane l < 16: entry l as last read
};
DEV SimdRank simdRankInit(uint32_t* tab, uint32_t stamp) {
    const uint32_t hw = (uint32_t)__builtin_amdgcn_s_getreg(4 | (31 << 11));        // HW_ID
    const uint32_t xcc = (uint32_t)__builtin_amdgcn_s_getreg(20 | (15 << 11)) & 7u;  // XCC_ID
    const uint32_t simd = (hw >> 4) & 3u, cu = (hw >> 8) & 15u, sh = (hw >> 12) & 1u, se = (hw >> 13) & 7u;
    const uint32_t key = (((xcc * 8u + se) * 2u + sh) * 16u + cu) * 4u + simd;
    SimdRank r;
    r.row = tab + (size_t)key * 16;
    r.me = (int)(hw & 15u);
    r.tag = (stamp & 0x7Fu) | 0x80u;
    r.seen = 0;
    return r;
}
// rank of estimate `est` among the entries read last time (ties: lower slot first), then post `est`
// and read the row again for the next call
DEV int simdRankStep(SimdRank& r, uint32_t est) {
    const int l = lane_id();
    est = est > 0xFFFFFFu ? 0xFFFFFFu : est;
    const uint32_t e = r.seen, ee = e & 0xFFFFFFu;
    const bool higher = l < 16 && l != r.me && (e >> 24) == r.tag && (ee > est || (ee == est && l < r.me));
    const int rank = __popcll(ballot(higher));
    if (l == 0) r.row[r.me] = (r.tag << 24) | est;
    r.seen = l < 16 ? __builtin_nontemporal_load(r.row + l) : 0u;
    return rank;
}

// Balanced game placement (multi-step c3 and c5 launches, KDyn.bal).  With the rank priority above the four
// games of a SIMD finish together, and a launch ends with its slowest SIMD: round 3 span data, a SIMD's
// end time correlates 0.86-0.96 with its games' total unit count and the slowest SIMD ends 8 % after the
// mean.  The dispatcher places blocks b, b + n/4, b + 2n/4, b + 3n/4 on one SIMD (one dispatch round of
// four waves per SIMD; identical in every launch and process measured; c5's 128-thread blocks: the game waves
// of b and b + n/2), so a permutation of games over blocks that gives each such group a heavy-to-light mix
// balances the SIMDs.  Each game posts its cost (units + own idle units) at the end of a launch; the last wave of each XCD class counting-sorts that class's posted
// counts and writes its part of the permutation for the next launches — snake order over the groups,
// so a group gets one game from each quarter of the order, heavy paired with light — and the stamp.  A launch whose predecessor on the
// handle left a permutation uses it (block b runs game perm[b]), else identity.  The permutation is
// sticky: only launches of at least BAL_MIN_ITER steps post costs and write a new one, shorter
// ones reuse the last (a game that changes CU pays cold TLB misses for its output pages: moving games
// at every launch cost a 20-step launch ~12 us, round 3 span data).  Which block runs a
// game never changes what the game computes: correctness needs only that perm is a permutation
// (a counting sort's output is one), and a missing or stale posted cost leaves the old stamp in place.
// c5 (partially observable 32x32 self-play with helper waves) is placed the same way, BAL_PO_GS games per group: the
// dispatcher puts the game waves of blocks b and b + n / 2 on one SIMD (round 6 span data,
// profiles/round6/placement_c5.json); c5 +0.6 %.
constexpr int BAL_MIN_ITER = 64, BAL_PO_GS = 2;
// an LDS pointer through an opaque scalar copy of its address: what is derived from it is register + offset
DEV uint8_t* ldsOpaque(uint8_t* p) {
    uint32_t a = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)p;
    asm volatile("" : "+s"(a));
    return (uint8_t*)(__attribute__((address_space(3))) uint8_t*)(uintptr_t)a;
}
DEV int balancedGame(const KDyn& D) {
    const int n = (int)gridDim.x;
    const int32_t hdr1 = __builtin_nontemporal_load(D.bal + 1);
    const int32_t pg = __builtin_nontemporal_load(D.bal + BAL_COST + n + (int)blockIdx.x);
    return hdr1 != 0 ? pg : (int)blockIdx.x;
}
DEV void balancePerm(const KDyn& D, uint32_t* hist, int c, int GS) {
    // games stay on their XCD: block b runs on XCD b % 8 and the four blocks of a SIMD group share b % 8,
    // so the permutation only moves games between blocks of the same residue class c (the state a game
    // left in that XCD's L2 stays near; round 6: one permutation over all games, balancing the XCDs' loads
    // too, was 1.2 % slower on c3 and -0.5 % on c5), and each class's LAST wave sorts that class alone: n / 8
    // games, n / 32 SIMD groups, the snake order as above (1/8 of the work on the launch's tail)
    // GS: games per SIMD group (c3: four game waves per SIMD; c5: BAL_PO_GS), blocks n / GS apart
    const int n = (int)gridDim.x, l = lane_id(), Q = (int)((uint32_t)n / (8u * (uint32_t)GS)), per = n >> 9;  // per: games per lane
    int32_t* const cost = D.bal + BAL_COST;
    int32_t* const perm = cost + n;
    const uint32_t tag = D.fwd_stamp & 0xFFFFu;
#pragma unroll
    for (int j = 0; j < 4; j++) hist[l + 64 * j] = 0;
    // this lane's games c + 8 * (l * per + i): all loads in flight at once, system scope (the costs
    // came through other XCDs' L2s)
    const __amdgpu_buffer_rsrc_t rs = bufRsrc(cost, (uint32_t)(n * 4));
    uint32_t cv[8];
#pragma unroll
    for (int i = 0; i < 8; i++)
        if (i < per) cv[i] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs, (int)((c + 8 * (l * per + i)) * 4), 0, 17);
    wsync();
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 8; i++)
        if (i < per) {
            ok = ok && (cv[i] >> 16) == tag;
            atomicAdd(&hist[255u - (cv[i] & 255u)], 1u);  // heaviest first
        }
    if (ballot(!ok)) return;  // a game has not posted (cannot happen: every wave posts before it counts): keep the old
    wsync();
    uint32_t v[4], sum = 0;  // exclusive prefix over the 256 bins: 4 per lane, then a wave scan
#pragma unroll
    for (int j = 0; j < 4; j++) {
        v[j] = hist[4 * l + j];
        sum += v[j];
    }
    const uint32_t incl = (uint32_t)wave_incl_sum((int)sum);
    uint32_t run = incl - sum;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        hist[4 * l + j] = run;
        run += v[j];
    }
    wsync();
#pragma unroll
    for (int i = 0; i < 8; i++)
        if (i < per) {
            const int r = (int)atomicAdd(&hist[255u - (cv[i] & 255u)], 1u);  // rank in the class
            const int q = r / Q, j = r - q * Q;
            perm[c + 8 * (q * Q + ((q & 1) ? Q - 1 - j : j))] = c + 8 * (l * per + i);
        }
    if (l == 0) D.bal[1] = (int32_t)D.fwd_stamp;  // (every class writes the same) the next launches take it
}

// Workgroup barrier for an LDS handoff: the release / acquire fences cover LDS only, so a wave does
// not drain its outstanding global stores at every step (a __syncthreads fence would).
DEV void ldsBarrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}
DEV void drainStores() { __builtin_amdgcn_s_waitcnt(0x0F70); }  // s_waitcnt vmcnt(0): this wave's stores done

// The helper wave of a partially observable HELP launch (32x32 self-play multi-step rollouts, BASELINE
// c5: two games per SIMD, the SIMD's vector issue half idle while the games run their dependent
// chains).  The render of both views (writeObsPOFast2, a third of the step's instructions) reads the
// state after the cycle and writes only the observation and the render record, so it moves to the
// helper: at step k the game wave packs the render inputs (packPO, double-buffered by step parity)
// and passes barrier B_k; the helper renders step k (renderPOPacked) while the game compacts, writes
// masks and the next rows and runs step k + 1, and is back at B_{k+1} before the game packs over
// the buffer it read.  The render record (sight rows, pending chunks) stays with the helper between
// steps; the game keeps the per-slot part (poRecordSnaps, the lane registers) as before.  A step the
// fast render cannot take (more than 64 units, sight > 15) the helper renders with the general
// writeObsPO straight from the game's live state while the game waits at a second barrier B'_k
// (the helper's stores, the global render record included, complete before it: the game re-reads
// that record in nextStep).  Only the helper ever writes the observation buffer, in step order; the
// game wave carries no render code.  The next step's snapshotBoth comes from the same pack: after
// B_k the helper first computes it (snapFromPack) and passes S_k, where the game, back from its
// compaction, masks and policy, takes the bytes (takeSnap), then renders step k.  Header flags: bit 2
// = packed render, bit 3 = general render from the live state.  Layout: hdr [2][4] words, the
// helper's view-0 sight rows [2][H] (the snapshot's rows before the render) and the snapshot bytes
// [64] at KDyn.help_off; the packs [2][5][64] words and the per-step occupant map (u8 per cell) in the
// game's `scell` area, which only the general render uses.
// After the snapshot bytes, at PO_HELP_REC words: the game's mask records of a packed step
// (writeMasksLanes with recOut: [5][64] words + a count word + 64 u16 vacated cells), stored by the
// helper after S_k (S_last after the last step), so the game wave issues none of those stores.
constexpr int PO_HELP_REC = 8 + 2 * 32 + 16, PO_HELP_REC_WORDS = 5 * 64 + 1 + 32;
template <class GameT>
DEV void helperLoopPO(GameT& G, uint32_t* hdr, int niter) {
    uint32_t* const rows0 = hdr + 8;
    uint8_t* const hsnap = (uint8_t*)(rows0 + 2 * G.H);
    uint8_t* const hcell = (uint8_t*)(G.scell + 2 * 5 * 64);
    uint32_t* const recs = hdr + PO_HELP_REC;
    G.helperLane();
    const int l = G.lid();
    for (int k = 0; k < niter; k++) {
        ldsBarrier();  // B_k
        const uint32_t* ph = hdr + (k & 1) * 4;
        const uint32_t f = uniu(ph[2]);
        const uint32_t* pk = G.scell + (k & 1) * 5 * 64;
        if (f & 4u) {
            if (k + 1 < niter) {
                G.snapFromPack(pk, ph, rows0, hsnap);
                ldsBarrier();  // S_k: the next step's snapshot bytes are ready
            }
            G.renderPOPacked(pk, ph, rows0, hcell, k == niter - 1);
            if (k + 1 == niter) ldsBarrier();  // S_last: the game's masks of the last step are out
            G.storeRecordsHelp(recs);  // step k's mask records and policy rows (written before S_k)
        } else if (f & 8u) {
            // the game's live state, as its own writeObsPO call would see it (the general render
            // overwrites `scell`, so the pack's record words are taken first)
            G.nu = (int)uniu(ph[0]);
            G.lcu = pk[192 + l];
            G.lkey = pk[256 + l];
            G.lsnap = (pk[128 + l] >> 8) & 0xFFu;
            for (int p = 0; p < 2; p++) G.writeObsPO(2 * G.g + p, p, ((f >> p) & 1u) != 0);
            drainStores();
            ldsBarrier();  // B'_k: the game continues (compaction)
        }
    }
}

template <int MODE, int FIX, int FCAP = 0, bool FPO = false, bool MULTI = false, bool HELP = false, bool LRI = false, bool STEADY = false>
// stateArg and PS lead the argument list so that kernarg preloading (-amdgpu-kernarg-preload-count,
// Makefile) hands them over in SGPRs: the first memory round (state block, unit-type table) issues
// without waiting for a scalar load of the kernel arguments.  The 16x16 instances (c3: four games per
// SIMD, at the 128-VGPR edge) and the helper instances are held to 4 waves per SIMD: one VGPR more
// silently halves nothing but drops a quarter of the games into a second dispatch round (1.7x slower).
__global__ __launch_bounds__(HELP ? 128 : 64, (HELP || FIX == 16) ? 4 : 1) void k_env(int32_t* __restrict__ stateArg, const KStatic* __restrict__ PS, KDyn D) {
    extern __shared__ __align__(16) uint8_t smemDyn[];
    // The steady instance addresses its LDS from an opaque copy of the base: one SGPR, and every array base of Game is
    // that register plus a constant, which folds into the ds_* offset field where the address is per lane.  From the
    // symbol itself each base is a constant of its own (`smem + offset`), materialised in an SGPR, hoisted out of the
    // step loop, spilled to a VGPR lane and read back in front of its uses (128 -> 117 VGPRs, no scratch;
    // the literal address 0 and a copy made again at every step were worse).
    uint8_t* const smem = STEADY ? ldsOpaque(smemDyn) : smemDyn;
    if (HELP && !FPO && threadIdx.x >= 64) {
        helperLoop(D, smem, (int)blockIdx.x, D.n_iter);
        return;
    }
    const KStatic& P = *PS;
    constexpr bool steady = STEADY;  // the D_* option tests below are constants in the steady instance
    // balanced placement (c3's and c5's multi-step kernels): this block's game from the previous launch's permutation
    // (balancePerm: a multiple of 512 games, at most 8 per lane and class)
    const bool balanced = MULTI && ((FIX == 16 && !FPO) || (FIX == 32 && FPO && HELP)) && D_HAS(bal) &&
                          (gridDim.x & 511) == 0 && gridDim.x <= 4096;
    const bool rebalance = balanced && D.n_iter >= BAL_MIN_ITER;  // this launch writes the next permutation
    const int game = balanced ? balancedGame(D) : -1;
    Game<STEADY> G(P, D, stateArg, FIX ? stateWords(FCAP, FIX * FIX) : D.state_words, smem, FIX ? FIX : D.H, FIX ? FIX : D.W, FIX ? FIX * FIX : D.HW, FIX ? FCAP : D.CAP,
           FIX ? FPO : P.partial_obs != 0, FIX ? 79 : P.utt.K, FIX ? 7 : P.utt.ntypes, FIX ? 7 : P.utt.maxAttackRadius, MULTI, game,
           FIX == 16 || FIX == 32);  // `walk`: the 16x16 instances (round 5) and c5's 32x32 (round 6: c5 +2.8 %)
    // the partially observable helper wave: one packed render per step (helperLoopPO)
    uint32_t* const poHelpHdr = (HELP && FPO) ? (uint32_t*)(smem + D.help_off) : nullptr;
    if (HELP && FPO && threadIdx.x >= 64) {
        helperLoopPO(G, poHelpHdr, D.n_iter);
        return;
    }
#ifdef MRTS_ABLATE
    G.G_AB = (uint32_t)g_ablate;
    const auto ab = [&G](int b) { return G.ab(b); };  // (the macros' bit test, as inside Game)
#endif
    // games [0, n_sp_games) are self-play (mrts_create's layout): no load needed to place the slots
    const bool selfplay = FIX ? true : G.g < D.n_sp_games;
    const int slot0 = selfplay ? 2 * G.g : 2 * D.n_sp_games + (G.g - D.n_sp_games);
    const int nslots = selfplay ? 2 : 1;
    // agent-vs-bot: the agent's side; bot-vs-bot: the side ai1 plays (JNIBotClient.gameStep(player))
    const int side = selfplay ? 0 : (D.players ? uni(D.players[slot0]) : 0);
    bool freshObs = true;  // observation comes from the current (post-step or fresh) state
#ifdef MRTS_PHASE_TIMING
#ifndef MRTS_SPAN_ONLY
    for (int i = 0; i < NPH; i++) G.phAcc[i] = 0;
#endif
    G.tph_ = __builtin_amdgcn_s_memtime();
    const uint64_t rt0_ = __builtin_amdgcn_s_memrealtime();
#endif

    if (MODE == MODE_RESET) {
        G.copyUtt();
        G.loadHeader(G.st());
        G.hset(H_KIND, P.game_kind[G.g]);
        G.hset(H_ERR, 0);
        G.initCells();
        G.storeTerrain();
        G.resetFromTemplate();
        if (D.mask_delta && D.masks) G.loadPrev();
        // JNIGridnetClientSelfPlay.reset zeroes reward/done slots j < rewards.length == 2 only
        // (tests/JNIGridnetClientSelfPlay.java:103-104,235-238): slots >= 2 keep the caller buffer's
        // previous values; JNIGridnetClient / JNIBotClient.reset zero every slot
        // (JNIGridnetClient.java:248-251, JNIBotClient.java:159-162)
        for (int k = lane_id(); k < nslots * D.n_rewards; k += 64) {
            if (selfplay && k % D.n_rewards >= 2) continue;
            if (D.reward) D.reward[(size_t)slot0 * D.n_rewards + k] = 0.0;
            if (D.done) D.done[(size_t)slot0 * D.n_rewards + k] = 0;
        }
    } else {
        G.load(D_ON(mask_delta) && D_HAS(masks));
        AB_ON(AB_LOAD, G.load(D_ON(mask_delta) && D_HAS(masks)));
    }
    // Multi-step launch (MULTI instances: mrts_rollout_fused_dev on the specialised full-observability
    // self-play shapes): the game runs D.n_iter consecutive fused steps with its state in LDS — each
    // iteration is one whole step (decode, issue, cycle, rewards, auto-reset, observation, masks, next
    // rows, all written to their buffers) — and stores the state once at the end.  A separate
    // instance: the loop changes register allocation (values live across iterations), and the
    // single-step kernels must not pay for it.
    const int kind = FIX ? GT_SELFPLAY : G.hget(H_KIND);
    const int gtype = kind & 15, ai1 = (kind >> 4) & 15, ai2 = (kind >> 8) & 15;
    const bool external = gtype != GT_BOT_VS_BOT;  // bot-only clients return no observation / masks
    // a game with a native LightRush side: the LRI instances of the generic step / reset kernels, which launchEnv
    // picks for the handles that have the bot's memory — every other handle runs kernels without the bot's code
    // (with it inlined behind cold branches, agent-vs-PassiveAI steps measured 1.8 % slower, §5l)
    constexpr bool LRK = LRI && FIX == 0 && (MODE == MODE_STEP || MODE == MODE_RESET);
    // (from the game's kind alone, which the state block's header holds: no KStatic load in a game without it —
    // mrts_create gives every handle with such a game the memory, KStatic.bot_off)
    const bool lr = LRK && ((gtype == GT_BOT_VS_BOT && (ai1 == GK_LIGHT_RUSH || ai2 == GK_LIGHT_RUSH)) ||
                            (gtype == GT_AGENT_VS_BOT && ai2 == GK_LIGHT_RUSH));
    if (MRTS_UNLIKELY(lr)) {
        G.lrInit(smem + P.bot_lds);
        if (MODE == MODE_RESET) G.lrClear();  // ai.reset() (JNIBotClient.java:149-167)
        else G.lrLoad();
    }
    const int niter = MULTI ? D.n_iter : 1;
#ifdef MRTS_PHASE_TIMING
    int nu0_ = 0;
#endif
    uint32_t* const helpBuf = (HELP && !FPO) ? (uint32_t*)(smem + D.help_off) : nullptr;  // helperLoop's layout
    bool poPacked = false;  // HELP && FPO: the previous iteration handed its render to the helper (packPO, flag 4)
    // c3 (four games per SIMD) only: on c5 the rank measured -4 % (its games outrank their own helper
    // waves, which then reach the handoff barriers late; round 3)
    const bool ranked = MULTI && FIX == 16 && D_HAS(prio_tab) && niter > 1;
    SimdRank srank;
    if (ranked) srank = simdRankInit(D.prio_tab, D.fwd_stamp);
    int oc = -1;  // steady: the carried outcome (MODE_STEP below)
    int rwKey = -1;  // steady: what the reward / done values last stored in this launch were made from (-1: none yet)
    if (HELP && !FPO) __syncthreads();  // A_0: the helper drew step 0's rows
    for (int it = 0; it < niter; it++) {
    if (it > 0) {
        AB_ON(AB_NEXTSTEP, G.ablNextStep());
        G.nextStep();
        freshObs = true;
    }
    // (the step body reads the by-value argument D, not the Game's per-iteration opaque pointer as its methods
    // do, freshLane: through the pointer SGPR spills went 153 -> 136 but c3 / c5 / c2 lost 0 to 0.6 %, the
    // re-read fields waiting on scalar loads where the spilled ones were a readlane; round 6)
    if (HELP && !FPO) G.helpRows = helpBuf + (it & 1) * 2 * 64;
    G.lastIt = it == niter - 1;
    G.firstIt = it == 0;
    bool snapTaken = false;
    if (MODE != MODE_RESET) {
        // Issue priority by game size: a SIMD runs several games at once and the kernel ends with its
        // slowest one, so the games with the most units (the longest serial chains) issue first.
        int q;
        constexpr int PRIO_T1 = 29, PRIO_T2 = 35, PRIO_T3 = 41;  // priority 1 / 2 / 3 from this many units + idle units
        if (FIX == 16) {
            // the c3 shape (four games per SIMD): units + own idle units (the step's decode / issue /
            // mask / policy work grows with the idle ones; against units alone at 24 / 30 / 36: c3 +1.8 % at
            // K = 200, +0.8 % at K = 20)
            // (steady: the count the previous step's writeMasksSteady took, Game::idleOwn — a launch's first step
            // and a step after one that wrote its masks the general way count here)
            int idle = steady ? G.idleOwn : -1;
            if (idle < 0) idle = (int)__popcll(ballot(G.lid() < G.nu && !(G.lua & UA_PRESENT) && uplay(G.lcu) >= 0));
            if (steady) G.idleOwn = -1;
            const int wq = G.nu + idle;
            q = wq >= PRIO_T3 ? 3 : wq >= PRIO_T2 ? 2 : wq >= PRIO_T1 ? 1 : 0;
            if (ranked) {  // from the second step on: the rank among the SIMD's waves by remaining work
                AB_ON(AB_PRIO, G.ablPrio(srank, RANK_C, niter - it));
                const int rk = simdRankStep(srank, (uint32_t)(wq + RANK_C) * (uint32_t)(niter - it));
                if (it > 0) q = 3 - (rk < 3 ? rk : 3);
            }
        } else {  // units (the idle count's ballot costs the latency-bound one-game-per-SIMD c2 4.5 %)
            // (c5, two games + their helper waves per SIMD: without any priority -9 %, the games all at 3 or all
            // above the helpers' 0 +-0.5 % — what counts is the games issuing before the helpers, round 6)
            q = G.nu >= 36 ? 3 : G.nu >= 30 ? 2 : G.nu >= 24 ? 1 : 0;
        }
        // c2's helper-wave launches: the game wave issues at priority >= 1, ahead of its helper wave (at 0) — round 6:
        // c2 +1.6 % / +0.4 % over two rounds of interleaved runs (the helper at 3 instead: -4.5 %); on c5 +0.5 % /
        // -0.6 %, so c5 keeps its unit-count priorities, which already put most of its games above their helpers
        if (HELP && !FPO) q = q < 1 ? 1 : q;
        if (q == 0) {
            if (it > 0) __builtin_amdgcn_s_setprio(0);
        } else if (q == 1) __builtin_amdgcn_s_setprio(1);
        else if (q == 2) __builtin_amdgcn_s_setprio(2);
        else __builtin_amdgcn_s_setprio(3);
    }
#ifdef MRTS_PHASE_TIMING
    if (it == 0) nu0_ = G.nu;
#endif
    if (G.po) G.clearSnap();
    if (HELP && FPO && poPacked) {  // S_{it-1}: the helper's snapshot of this step (snapFromPack)
        ldsBarrier();
        G.takeSnap((const uint8_t*)(poHelpHdr + 8 + 2 * G.H));
        snapTaken = true;
    }
    PHASE(0);

    if (MODE == MODE_PLAYOUT) {
        // NaiveMCTS.simulate (ai/mcts/naivemcts/NaiveMCTS.java:297-308, the same loop as
        // ai/AALL/mcts/ModelledEvaluationMCTS.java:313-324): do { if (isComplete()) gameover = cycle();
        // else { issue(policy.getAction(0)); issue(policy.getAction(1)); } } while (!gameover &&
        // time < until).  The policies give every idle unit an action, so after an issue pass the
        // state is complete: one pass below = [issue pass if incomplete] + cycle.  The state stays in
        // LDS for the whole playout; time grows by one per pass, so every wave reaches the exit.
        const int until = G.time + D.horizon;
        bool first = true;
        for (;;) {
            if (!G.complete()) {
                aiGetAction(G, ai1, 0);
                G.issuePlayer(0, 10, true);
                aiGetAction(G, ai2, 1);
                G.issuePlayer(1, 10, true);
                if (first && G.time >= until) break;  // the do-while's first test follows the issue pass
            }
            first = false;
            G.cycle();
            bool over;
            int winner;
            G.outcome(over, winner);
            if (G.deaths) {
                G.compact();
                G.deaths = 0;
            }
            if (over || G.time >= until) break;
        }
        wsync();
        G.store();
        return;
    }

    if (MODE == MODE_TRACE) {
        // TestTracesIntegrity.testTrace (test/microrts/TestTracesIntegrity.java:72-127), one entry per
        // launch: issueSafe(p0's pairs), issueSafe(p1's pairs) (:119-120), then GameState.cycle() until
        // the next entry's time (:83-86).  The Java asserts that no cycle follows a cycle that ended the
        // game; cycle() returns gameover() of the state it leaves, which is this state again before the
        // next cycle (issuing moves no unit) — so a game over before any further cycle is that failure.
        uint32_t flags = 0;
        const int32_t* rows = D.rows + (size_t)G.g * D.n_rows * 8;
        const bool i0 = G.traceIssue(0, rows, D.n_rows, flags);
        const bool i1 = G.traceIssue(1, rows, D.n_rows, flags);
        if (i0 || i1) flags |= TR_ISSUED;
        const int until = uni(D.trace_until[G.g]);
        while (G.time < until) {
            if (G.time > 0) {
                bool over;
                int winner;
                G.outcome(over, winner);
                if (over) {
                    flags |= TR_GAMEOVER;
                    break;
                }
            }
            G.cycle();
            if (G.deaths) {
                G.compact();
                G.deaths = 0;
            }
        }
        wsync();
        G.store();
        if (lane_id() == 0) D.trace_out[G.g] = (int32_t)flags;
        return;
    }

    if (MODE == MODE_STEP) {
        const size_t rowStride = (size_t)G.HW * 7;
        // fused uniform policy: this step's rows go out first (fire-and-forget stores, nothing in the
        // launch reads them back: fetchRow draws the idle units' rows again)
        if (D_OFF(uni_actions) && !(HELP && !FPO)) G.writeUniformRows(slot0, nslots);
        if (MRTS_UNLIKELY(D_ZERO(reward_need) & RN_COUNTS))
            if (lane_id() < 2 * RC_N) G.rwc[lane_id()] = 0;
        if (MRTS_UNLIKELY(D_ZERO(reward_need) & RN_CLOSER)) G.closerBefore();
        const bool rowsMode = FIX ? false : D.rows != nullptr;
        if (rowsMode && gtype == GT_SELFPLAY) {
            for (int p = 0; p < 2; p++) {
                if (G.po) G.snapshot(p);
                const int np = G.rowsDecode(p, D.rows + (size_t)(slot0 + p) * D.n_rows * 8);
                G.rowsIssue(p, np, 1);
            }
        } else if (rowsMode && gtype == GT_AGENT_VS_BOT) {
            if (G.po) {
                G.snapshot(side);
                G.snapshot(1 - side);
            }
            const int np = G.rowsDecode(side, D.rows + (size_t)slot0 * D.n_rows * 8);
            aiGetAction<LRK>(G, ai2, 1 - side);
            G.rowsIssue(side, np, 1);
            aiIssue<LRK>(G, ai2, 1 - side);
        } else if (gtype == GT_SELFPLAY) {
            // JNIGridnetClientSelfPlay.gameStep (tests/JNIGridnetClientSelfPlay.java:159-189)
            if (MRTS_LIKELY(G.nu <= 64 && (!G.po || G.snapBothOk()))) {
                G.selfPlayFast(D.actions + (size_t)slot0 * rowStride, D.actions + (size_t)(slot0 + 1) * rowStride, slot0,
                               snapTaken);
            } else {
            G.predecode(D.actions + (size_t)slot0 * rowStride, D.actions + (size_t)(slot0 + 1) * rowStride, -1, slot0, slot0 + 1);
            PHASE(1);
            const bool snapBoth = G.po && G.snapBothOk();
            for (int p = 0; p < 2; p++) {
                if (snapBoth) {
                    if (p == 0 && !snapTaken) G.snapshotBoth();
                    else G.snapshotActions(1);
                } else if (G.po) {
                    G.snapshot(p);
                }
                if (G.nu <= 64) {
                    G.decode(p, true);
                } else {
                    G.decode(p);
                    PHASE(2);
                    G.issuePlayer(p, 1, false);
                }
                PHASE(3);
            }
            }
        } else if (gtype == GT_AGENT_VS_BOT) {
            // JNIGridnetClient.gameStep (tests/JNIGridnetClient.java:163-203): both views are taken and
            // both actions computed before either issueSafe
            const int32_t* rows = D.actions + (size_t)slot0 * rowStride;
            G.predecode(rows, rows, side, slot0, slot0);
            if (G.po) {
                G.snapshot(side);
                G.snapshot(1 - side);
            }
            G.decode(side);
            aiGetAction<LRK>(G, ai2, 1 - side);
            G.issuePlayer(side, 1, false);
            aiIssue<LRK>(G, ai2, 1 - side);
        } else {
            // JNIBotClient.gameStep (tests/JNIBotClient.java:108-135): both AIs on the full state
            aiGetAction<LRK>(G, ai1, side);
            aiGetAction<LRK>(G, ai2, 1 - side);
            aiIssue<LRK>(G, ai1, side);
            aiIssue<LRK>(G, ai2, 1 - side);
        }
        G.cycle();
        PHASE(4);
        bool gameover;
        int winner;
        // (in the form it had, writeRewards on the steady instance too — there it writes the WinLoss pair, R = 1 and kind 0
        // being what a steady launch has: with the pair stored by a member of the copies' section the steady instance
        // spilled two VGPRs)
        AB_ON(AB_OUTCOME, G.outcome(gameover, winner); G.writeRewards(slot0, nslots, selfplay ? 0 : side, selfplay ? 1 : side, gameover, winner));
        if (steady) {
            // gameover / winner change only when a unit dies or the game is reset (a PRODUCE adds a unit to a player
            // that has one): carried between the steps of the launch (oc: winner + 1 | gameover << 2, -1 = not known)
            if (oc < 0 || G.deaths) {
                G.outcome(gameover, winner);
                oc = (winner + 1) | (gameover ? 4 : 0);
            }
            gameover = (oc & 4) != 0;
            winner = (oc & 3) - 1;
        } else {
            G.outcome(gameover, winner);
        }
        // reward functions + VecClient auto-reset on done[0] or max steps, keeping the terminal
        // reward/done and forcing done[0] (tests/JNIGridnetVecClient.java:214-287)
        const int steps = G.hget(H_STEPS) + 1;
        G.hset(H_STEPS, steps);
        bool reset;
        if (steady) {
            // WinLoss alone into the plain per-handle buffers (writeRewards' first branch and the forced done[0]
            // below, in one store each): the values are a function of (gameover, winner, reset), and the buffers
            // persist from step to step, so they are stored on the launch's first step (whatever the caller left
            // there) and whenever that triple differs from the last one stored — a game over, an auto-reset, or the
            // step after either.  After every step the buffers hold what a full write would.
            reset = gameover || steps >= D.max_steps;
            const int key = (gameover ? oc : 0) | (reset ? 8 : 0);
            if (key != rwKey && lane_id() < 2) {
                D.reward[slot0 + lane_id()] = gameover ? (winner == lane_id() ? 1.0 : -1.0) : 0.0;
                D.done[slot0 + lane_id()] = reset ? 1 : 0;
            }
            rwKey = key;
            AB_ON(AB_REWARD, G.ablRewardStores(slot0, gameover, winner, reset));
        } else {
            const bool done0 = G.writeRewards(slot0, nslots, selfplay ? 0 : side, selfplay ? 1 : side, gameover, winner, it);
            reset = done0 || steps >= D.max_steps;
            if (reset && D.done != nullptr && lane_id() < nslots)
                D.done[(size_t)((uint32_t)it * (uint32_t)D.resp_stride) + (size_t)(slot0 + lane_id()) * D.n_rewards] = 1;
        }
        if (MRTS_UNLIKELY(reset)) {
            G.hset(H_STEPS, 0);  // envSteps[i] = 0 (JNIGridnetVecClient.java:229,264-265,285)
            G.resetFromTemplate();
            // the walls of the env's own map too, whatever the block held (a state injected as JSON may have brought
            // other terrain; resetFromTemplate keeps the cell map's walls)
            // (the 8x8 helper wave is the second writer of its games' observations: there the terrain plane is the
            // helper's to store, told by this step's pack — packObs(buf, true) below — and no store from here races it)
            const bool ownObs = D_HAS(obs) && external && !(HELP && !FPO);
            restoreMapTerrain(G.cell, G.tmpl() + T_TERR, G.st() + stateTerrOff(G.CAP, G.HW),
                              ownObs ? D.obs + ((size_t)slot0 * D.C + 5) * G.HW : nullptr, nslots, D.C * G.HW, G.HW, G.lid());
            wsync();
            if (steady) oc = -1;
            if (G.po) G.clearSnap();
            if (MRTS_UNLIKELY(lr)) G.lrClear();  // the auto-reset resets the AIs too (JNIBotClient.java:149-167)
        } else {
            freshObs = false;
        }
        PHASE(5);
    }

    uint32_t poHelpFlags = 0;  // HELP && FPO: bit 2 = the helper renders this step, bit 3 = the game does
    if (MODE != MODE_MASKS && D_HAS(obs) && external) {
        if (G.po) {
            // persistent buffer: the views the previous write rendered for this game can be updated
            // in place (writeObsPO's delta)
            const bool canDelta = MODE == MODE_STEP && !freshObs && D.obs_delta && D.po_prev && poDeltaShape(G.H, G.W) &&
                                  G.nu <= 64 && G.hget(H_NU) <= 64;
            const uint32_t valid = canDelta ? (uint32_t)G.hget(Game<STEADY>::HX_POVALID) : 0u;
            if (selfplay && G.poFast2()) {
                if (freshObs) {  // PO views of the reset state (snapshot(p) touches only view p's bits)
                    if (G.snapBothOk()) {
                        G.snapshotBoth();
                        G.snapshotActions(1);
                    } else {
                        G.snapshot(0);
                        G.snapshot(1);
                    }
                }
                if (HELP && FPO) {
                    G.packPO(G.scell + (it & 1) * 5 * 64, poHelpHdr + (it & 1) * 4, valid & 3u, 4u);
                    poHelpFlags = 4u;
                } else
                AB_SKIP(AB_SKIP_OBS)
                G.writeObsPOFast2(slot0, valid & 3u);
            } else if (HELP && FPO) {
                // the helper renders from the live state while this wave waits at B'_it (below)
                if (freshObs) {
                    G.snapshot(0);
                    G.snapshot(1);
                }
                G.packPO(G.scell + (it & 1) * 5 * 64, poHelpHdr + (it & 1) * 4, valid & 3u, 8u);
                poHelpFlags = 8u;
            } else
            for (int i = 0; i < nslots; i++) {
                const int p = selfplay ? i : side;
                if (freshObs) G.snapshot(p);  // PO view of the reset state
                AB_SKIP(AB_SKIP_OBS)
                G.writeObsPO(slot0 + i, p, ((valid >> p) & 1u) != 0);
            }
        } else if (HELP) {
            // the helper wave renders it; after an auto-reset (freshObs) with the terrain plane, as on the first step
            G.packObs(helpBuf + 2 * 2 * 64 + (it & 1) * 2 * 64, MODE == MODE_STEP && freshObs);
        } else {
            AB_SKIP(AB_SKIP_OBS)
            G.writeObsFull(slot0, nslots, side);
            AB_ON(AB_OBS, G.writeObsFull(slot0, nslots, side));
        }
    }
    if (MODE == MODE_STEP && MRTS_UNLIKELY(D_OFF(rec_out) != nullptr) && external) G.writeRecord(it);
    if (HELP && !FPO) __syncthreads();  // A_{it+1}: step it's cells packed; the helper's rows of step it + 1 ready
    if (HELP && FPO) {
        if (poHelpFlags == 0u && G.lid() == 0) poHelpHdr[(it & 1) * 4 + 2] = 0u;
        ldsBarrier();  // B_it: the helper takes step it's pack (helperLoopPO)
        if (poHelpFlags == 8u) ldsBarrier();  // B'_it: the helper rendered from this wave's live state
        poPacked = poHelpFlags == 4u;
    }
    PHASE(6);
    if (MODE == MODE_STEP && !freshObs && G.deaths) {
        if (MRTS_UNLIKELY(lr)) G.lrCompact();
        G.compact();
        if (steady) AB_ON(AB_COMPACT_STEADY, G.compact());  // once more: no dead slot is left, every unit keeps its place
    }
    PHASE(7);
    if (HELP && FPO) {  // a packed step's mask records go to the helper (storeRecordsHelp)
        G.recOut = poHelpFlags == 4u ? poHelpHdr + PO_HELP_REC : nullptr;
        if (poHelpFlags == 4u && G.lid() == 0) G.recOut[5 * 64] = 0u;  // none, unless writeMasksLanes hands them over
    }
    if (D_HAS(masks) && external) {
        const int nsl = selfplay ? 2 : 1;
        if (MRTS_LIKELY(D_ON(mask_delta) && G.nu <= 64 && nsl * maskWords(G.HW) <= 64 && G.K <= 96)) {
            PHASE(8);
            if constexpr (steady) G.writeMasksSteady(slot0);
            else if (selfplay) G.writeMasksLanes(slot0, 2, 0, 1);
            else G.writeMasksLanes(slot0, 1, D.mask_player, D.mask_player);
        } else {
        wsync();
        G.stashMasks(selfplay ? 3 : (1 << D.mask_player));
        wsync();
        PHASE(8);
        if (selfplay) G.writeMasks(slot0, 2, 0, 1);
        else G.writeMasks(slot0, 1, D.mask_player, D.mask_player);
        }
        if (D_HAS(pol_actions) && !(D_ON(pol_delta) && D_ON(mask_delta) && ((G.HW * G.K) & 15) == 0)) {  // no dirty-row pass ran
            wsync();
            if (selfplay) G.writePolicyAll(slot0, 2, 0, 1);
            else G.writePolicyAll(slot0, 1, D.mask_player, D.mask_player);
        }
        PHASE(9);
    }
    if (MODE != MODE_MASKS && G.po && D.obs && external && D.po_prev && poDeltaShape(G.H, G.W)) {
        wsync();
        G.poRecordSnaps(selfplay ? 3u : (1u << side));
    }
    if (HELP && FPO && poPacked && it == niter - 1) ldsBarrier();  // S_last (helperLoopPO)
    }  // iterations
    if (ranked && lane_id() == 0) srank.row[srank.me] = 0u;  // this game no longer competes on its SIMD
    if (MODE != MODE_MASKS) {
        wsync();
        G.store();
        AB_ON(AB_STORE, G.store());
        if (MRTS_UNLIKELY(lr)) G.lrStore();
    }
    if (rebalance) {  // post this game's final unit count; the launch's LAST wave writes the next placement
        const uint32_t tag = D.fwd_stamp & 0xFFFFu;
        uint32_t last = 0;
        // the cost posted for the next placement: units + own idle units at the launch's last step, the estimate
        // the SIMD rank uses (round 6, against the unit count: c3 K = 20 kernel -0.6 %, c5 +0.4 %; the estimate
        // averaged over the launch's steps was worse)
        const int cost = G.nu + (int)__popcll(ballot(G.lid() < G.nu && !(G.lua & UA_PRESENT) && uplay(G.lcu) >= 0));
        if (lane_id() == 0) {
            // agent scope, written through: the last wave may sit on another XCD (another L2)
            __hip_atomic_store(D.bal + BAL_COST + G.g, (int32_t)((tag << 16) | (uint32_t)(cost < 255 ? cost : 255)),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            drainStores();  // the cost is in memory before this wave counts itself
            // waves of this block's class (b % 8) finished in this launch, wrapping to 0 at the last
            // (atomicInc): no reset needed, and no compare-and-swap retries (4096 contending CAS loops
            // at device scope took milliseconds)
            const uint32_t old = atomicInc((uint32_t*)D.bal + 2 + (blockIdx.x & 7u), gridDim.x / 8u - 1u);
            last = old == gridDim.x / 8u - 1u ? 1u : 0u;
        }
        if (uniu(last)) {
            wsync();
            balancePerm(D, (uint32_t*)smem, (int)(blockIdx.x & 7u), FIX == 16 ? 4 : BAL_PO_GS);
        }
    }
    PHASE(10);
#ifdef MRTS_PHASE_TIMING
    if (lane_id() == 0 && G.g < PH_GAMES) {
#ifndef MRTS_SPAN_ONLY
        for (int i = 0; i < NPH; i++) g_phase[i * PH_GAMES + G.g] += G.phAcc[i];
#endif
#ifdef MRTS_NO_MILESTONES
        // odd launch stamps go to blocks 3 / 4 (free without milestones): two back-to-back launches
        // can be compared (tools/launch_gap.py)
        const int sb_ = (D.fwd_stamp & 1u) ? 3 : 0;
#else
        const int sb_ = 0;
#endif
        g_span[sb_ * PH_GAMES + G.g] = rt0_;
        g_span[(sb_ + 1) * PH_GAMES + G.g] = __builtin_amdgcn_s_memrealtime();
        g_span[2 * PH_GAMES + G.g] = (unsigned long long)(uint32_t)__builtin_amdgcn_s_getreg(4 | (31 << 11)) |
                                     ((unsigned long long)(__builtin_amdgcn_s_getreg(20 | (15 << 11)) & 15) << 32) |
                                     ((unsigned long long)(nu0_ & 255) << 40) | ((unsigned long long)(G.nu & 255) << 48);
    }
#endif
}

#ifdef MRTS_LANE_AUDIT
// the audit's negative control: a readlane of lane 40 from a branch only lanes 0..31 take
__global__ __launch_bounds__(64) void k_lane_audit_probe(int32_t* out) {
    int v = 0;
    if (threadIdx.x < 32) v = rl((int)threadIdx.x * 3, 40);
    out[threadIdx.x] = v;
}
#endif
}  // namespace

namespace mrts {
#ifdef MRTS_LANE_AUDIT
hipError_t laneAuditProbe(int32_t* scratch) {
    hipLaunchKernelGGL(k_lane_audit_probe, dim3(1), dim3(64), 0, 0, scratch);
    return hipGetLastError();
}
// out[256]: per thread slot the last violation of any unit (source line | unit << 20 | kind << 24: 1 readlane, 2 DPP,
// 3 ballot), 0 = none
hipError_t laneAudit(int32_t* out, int reset) {
    std::fill(out, out + 256, 0);
    hipError_t e = laneAuditUnit<0>(out, reset);
    if (e == hipSuccess) e = laneAuditUnit<1>(out, reset);
    if (e == hipSuccess) e = laneAuditUnit<2>(out, reset);
    return e;
}
#endif
#ifdef MRTS_ABLATE
hipError_t setAblate(uint64_t v) { return hipMemcpyToSymbol(HIP_SYMBOL(g_ablate), &v, sizeof(v)); }
hipError_t getDbg(unsigned long long* out, int reset) {
    hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_dbg), sizeof(unsigned long long) * 4);
    if (e == hipSuccess && reset) {
        unsigned long long z[4] = {0, 0, 0, 0};
        e = hipMemcpyToSymbol(HIP_SYMBOL(g_dbg), z, sizeof(z));
    }
    return e;
}
#endif
#ifdef MRTS_PHASE_TIMING
// out[16]: per-phase sums over games (and the max over games in out[16..31] when given 32 slots)
hipError_t phaseTimes(unsigned long long* out, int reset) {
    std::vector<unsigned long long> h((size_t)NPH * PH_GAMES);
    hipError_t e = hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(g_phase), h.size() * sizeof(h[0]));
    if (e != hipSuccess) return e;
    for (int i = 0; i < NPH; i++) {
        unsigned long long sum = 0, mx = 0;
        for (int g = 0; g < PH_GAMES; g++) {
            sum += h[(size_t)i * PH_GAMES + g];
            mx = h[(size_t)i * PH_GAMES + g] > mx ? h[(size_t)i * PH_GAMES + g] : mx;
        }
        out[i] = sum;
        out[NPH + i] = mx;
    }
    if (reset) {
        std::fill(h.begin(), h.end(), 0ull);
        e = hipMemcpyToSymbol(HIP_SYMBOL(g_phase), h.data(), h.size() * sizeof(h[0]));
    }
    return e;
}
hipError_t phaseSpans(unsigned long long* out, int n) {  // [11][n]: starts, ends, placements, milestones of the last launch
    std::vector<unsigned long long> h((size_t)11 * PH_GAMES);
    hipError_t e = hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(g_span), h.size() * sizeof(h[0]));
    if (e != hipSuccess) return e;
    for (int b = 0; b < 11; b++)  // starts, ends, placements, then the span build's 8 milestones
        for (int i = 0; i < n && i < PH_GAMES; i++) out[(size_t)b * n + i] = h[(size_t)b * PH_GAMES + i];
    return e;
}
#endif
// The dynamic LDS sizes.  Game's constructor and Game::lrInit carve the arrays; these two functions are the only other
// copy of the layout, written in the carvers' order, one term per array, so the two can be read side by side (the
// carvers stay as they are: taking their pointers from a shared description changed the step kernels' code).
// LDS of the native LightRush after the game's own (Game::lrInit)
size_t lrLdsBytes(int HW, int W, int CAP) {
    const size_t NB2 = (size_t)((HW + 2 * W + 31) / 32);
    size_t q = 4 * (size_t)botWords(CAP);  // lrMem
    q += 4 * (size_t)HW;                   // lrKey
    q += 3 * 4 * NB2;                      // lrGs, lrRu, lrPa
    q += 4 * (size_t)maskWords(HW);        // lrFree
    q += 3 * 2 * (size_t)HW;               // lrCell, lrPar, lrCost
    q += 2 * 2 * (size_t)CAP;              // lrOrd [2][CAP]
    return q;
}
size_t ldsBytes(int HW, int W, int CAP, int po) {
    const size_t H = (size_t)(HW / W), NCW = (size_t)poChunkWords(HW);
    size_t q = UTT_LDS;                             // the unit-type table copy
    q += 4 * 4 * (size_t)CAP;                       // uc, ua, at, as
    q += 4 * (size_t)((HW + 2 * W + 31) / 32);      // bits
    q += 4 * 64;                                    // rseq
    q += 8 * (size_t)maskWords(HW);                 // mprev
    q += 4 * 16 + 4 * 32;                           // rwc, hdr
    q += 3 * 2 * (size_t)CAP;                       // hp, res, par
    q += 2 * (size_t)HW + 2 * 64;                   // cell, rslot
    const size_t snapBytes = ((size_t)CAP + 3) & ~(size_t)3;
    if (!po)  // snap — on 16x16 under the observation byte image writeObsFullImg lays over it (5 planes of HW bytes)
        return q + std::max(snapBytes, HW == 256 ? 5 * (size_t)HW : (size_t)0);
    q += snapBytes;
    q += 4 * (size_t)HW + 4 * 2 * H * (size_t)((W + 31) / 32);  // scell, vis
    if (poDeltaShape((int)H, W)) {
        q += 4 * (4 * H + 2 * NCW + 4 * NCW + 2 * H);  // poVis, poPend, poDirty, vis2
        q += 4 * (size_t)((HW / 4 + 1) & ~1);          // poList
    }
    return q;
}
// what follows the game's own LDS starts at the next 16-byte boundary: the LightRush area (KStatic.bot_lds), or a
// HELP instance's helper-wave area (KDyn.help_off) of HELP8_LDS (helperLoop's rows) / HELP32PO_LDS (helperLoopPO's
// header and record words) bytes
static size_t ldsAlign16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }
constexpr size_t HELP8_LDS = 2048, HELP32PO_LDS = 4 * (PO_HELP_REC + PO_HELP_REC_WORDS);
size_t ldsLightRushOff(int HW, int W, int CAP, int po) { return ldsAlign16(ldsBytes(HW, W, CAP, po)); }
size_t handleLdsBytes(int HW, int W, int CAP, int po, bool lightRush) {
    return lightRush ? ldsLightRushOff(HW, W, CAP, po) + lrLdsBytes(HW, W, CAP) : ldsBytes(HW, W, CAP, po);
}

// The shapes with specialised k_env instances (the sizes are constants in them; each has single-step, MULTI and
// MODE_TRACE instances but S32PO, which has no MODE_TRACE one) and the condition common to them: the unit-type table
// the constants were compiled for, a square map, and every game self-play.
enum { S16 = 0, S8 = 1, S32PO = 2 };
constexpr struct { int W, CAP; bool po; } SPEC_SHAPES[3] = {{16, 320, false}, {8, 128, false}, {32, 320, true}};
// index into SPEC_SHAPES, or -1: the generic instances.  anyKind: MODE_TRACE's selection — it steps single games of
// a forward-model handle through the specialised games' code whatever their kind, so it ignores n_sp_games.
static int specialisedShape(const KStatic& hs, bool anyKind = false) {
    if (!(anyKind || hs.n_sp_games == hs.n_games) || hs.utt.K != 79 || hs.utt.ntypes != 7 || hs.utt.maxAttackRadius != 7 || hs.H != hs.W)
        return -1;
    for (int i = 0; i < 3; i++)
        if (hs.W == SPEC_SHAPES[i].W && hs.CAP == SPEC_SHAPES[i].CAP && (hs.partial_obs != 0) == SPEC_SHAPES[i].po) return i;
    return -1;
}
// The generic instances take any map, so theirs is the LDS that can exceed the default limit (the specialised
// shapes' never does): the attribute is set on every instance envInstance returns for shape -1.
hipError_t prepareLds(size_t bytes) {
    hipError_t e = hipFuncSetAttribute((const void*)k_env<MODE_STEP, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_env<MODE_RESET, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_env<MODE_MASKS, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_env<MODE_PLAYOUT, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_env<MODE_TRACE, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess)
        e = hipFuncSetAttribute((const void*)k_env<MODE_STEP, 0, 0, false, false, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess)
        e = hipFuncSetAttribute((const void*)k_env<MODE_RESET, 0, 0, false, false, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    return e;
}

// e0 / e1 (may be null): timing events the launch records itself (hipExtLaunchKernelGGL: the kernel
// dispatch's own start / end timestamps — no separate marker packets around it; mrts_set_rollout_events)
// The steady state of the fused self-play rollout on the 16x16 shape (BASELINE c3's launch): a multi-step launch whose
// masks, policy rows and action rows all continue the previous launch's, with the plain int32 observation, WinLoss
// alone as the reward and none of the optional outputs.  k_env's STEADY instance compiles these tests as constants
// (D_HAS / D_OFF / D_ON / D_ZERO), so every condition below is one the instance relies on: a launch that deviates in
// any of them runs the general instance.  (KDyn.players is not among them: the specialised self-play instances never
// read it, and the Python front end always passes its players tensor.)
static bool steadyLaunch(const KStatic& hs, const KDyn& D) {
    const bool shape = specialisedShape(hs) == S16 && !hs.bot_off;
    const bool on = D.n_iter > 1 && D.mask_delta == 1 && D.pol_delta == 1 && D.fwd_read == 1 && D.obs_img == 1;
    const bool has = D.actions && D.obs && D.masks && D.source && D.pol_actions && D.reward && D.done && D.prio_tab && D.bal;
    const bool off = !D.obs8 && !D.obs16 && !D.rec_out && !D.uni_actions && !D.rows;
    const bool zero = D.resp_stride == 0 && D.n_rewards == 1 && D.reward_kinds4 == (uint32_t)RF_WINLOSS && D.reward_need == 0;
    return shape && on && has && off && zero;
}
// steadyLaunch for a launch that deviates from the steady state in one condition (`dev` < 0: in none): 1 / 0, or -1
// past the last deviation.  Not part of include/mrts.h: the tests' view of the selection.
static int32_t g_probeBuf[4];
// the steady state's launch arguments (the probes below deviate from them); `some`: a non-null buffer
static KDyn steadyDyn() {
    void* const some = g_probeBuf;
    KDyn D{};
    D.n_iter = 20;
    D.mask_delta = D.pol_delta = D.fwd_read = D.obs_img = 1;
    D.actions = (const int32_t*)some;
    D.obs = (int32_t*)some;
    D.masks = (uint8_t*)some;
    D.source = (uint32_t*)some;
    D.pol_actions = (int32_t*)some;
    D.reward = (double*)some;
    D.done = (uint8_t*)some;
    D.prio_tab = (uint32_t*)some;
    D.bal = (int32_t*)some;
    D.n_rewards = 1;
    return D;
}
extern "C" int mrts_internal_steady_probe(int dev) {
    KStatic hs{};
    hs.n_games = hs.n_sp_games = 512;
    hs.utt.K = 79;
    hs.utt.ntypes = 7;
    hs.utt.maxAttackRadius = 7;
    hs.H = hs.W = 16;
    hs.HW = 256;
    hs.CAP = 320;
    void* const some = g_probeBuf;
    KDyn D = steadyDyn();
    switch (dev) {
        case 0: D.n_iter = 1; break;
        case 1: hs.H = hs.W = 8; hs.HW = 64; hs.CAP = 128; break;
        case 2: hs.partial_obs = 1; break;
        case 3: hs.n_games = 513; break;
        case 4: hs.bot_off = 1; break;
        case 5: D.mask_delta = 0; break;
        case 6: D.pol_delta = 0; break;
        case 7: D.fwd_read = 0; break;
        case 8: D.obs_img = 0; break;
        case 9: D.obs = nullptr; break;
        case 10: D.masks = nullptr; break;
        case 11: D.source = nullptr; break;
        case 12: D.pol_actions = nullptr; break;
        case 13: D.reward = nullptr; break;
        case 14: D.done = nullptr; break;
        case 15: D.prio_tab = nullptr; break;
        case 16: D.bal = nullptr; break;
        case 17: D.obs8 = (uint8_t*)some; break;
        case 18: D.obs16 = (int16_t*)some; break;
        case 19: D.rec_out = (uint32_t*)some; break;
        case 20: D.uni_actions = (int32_t*)some; break;
        case 21: D.rows = (const int32_t*)some; break;
        case 22: D.resp_stride = 1024; break;
        case 23: D.n_rewards = 2; break;
        case 24: D.reward_kinds4 = (uint32_t)RF_ATTACK; break;
        case 25: D.reward_need = RN_COUNTS; break;
        case 26: D.actions = nullptr; break;
        default: if (dev >= 0) return -1;
    }
    return steadyLaunch(hs, D) ? 1 : 0;
}

// The instance of k_env a launch runs.  The three selections below start from the one shape test and differ in two
// things: rows (mrts_step_rows' per-unit rows in place of the action tensor) is a MODE_STEP argument the specialised
// step instances do not read, so it sends a step to the generic instance and concerns no other mode; and MODE_TRACE
// steps single games of a forward-model handle, of any kind, so it ignores n_sp_games (and rows: it has none).
enum EnvInst { EI_STEADY16, EI_MULTI16, EI_STEP16, EI_HELP8, EI_MULTI8, EI_STEP8, EI_HELP32PO, EI_MULTI32PO, EI_STEP32PO,
               EI_STEP_LR, EI_STEP, EI_RESET_LR, EI_RESET, EI_PLAYOUT, EI_TRACE16, EI_TRACE8, EI_TRACE, EI_MASKS };
static EnvInst envInstance(int mode, const KStatic& hs, const KDyn& D) {
    switch (mode) {
        case MODE_STEP: {
            const int s = D.rows == nullptr ? specialisedShape(hs) : -1;
            const bool multi = D.n_iter > 1;
            if (s == S16) return steadyLaunch(hs, D) ? EI_STEADY16 : multi ? EI_MULTI16 : EI_STEP16;
            // c2's fused uniform rollout: a helper wave per game (helperLoop)
            if (s == S8) return !multi ? EI_STEP8 : (D.uni_actions && !D.masks) ? EI_HELP8 : EI_MULTI8;
            // c5's partially observable rollout: a helper wave per game renders the views (helperLoopPO)
            if (s == S32PO) return !multi ? EI_STEP32PO : (D.obs && !MRTS_NO_PO_HELPER) ? EI_HELP32PO : EI_MULTI32PO;
            return hs.bot_off ? EI_STEP_LR : EI_STEP;
        }
        case MODE_RESET: return hs.bot_off ? EI_RESET_LR : EI_RESET;
        case MODE_PLAYOUT: return EI_PLAYOUT;
        case MODE_TRACE: {
            // the specialised 16x16 / 8x8 step instances' dimensions (their games' code with constant
            // sizes), else the generic kernel
            const int s = D.trace_generic ? -1 : specialisedShape(hs, true);
            return s == S16 ? EI_TRACE16 : s == S8 ? EI_TRACE8 : EI_TRACE;
        }
        default: return EI_MASKS;
    }
}
hipError_t launchEnv(int mode, const KStatic& hs, const KStatic* ds, const KDyn& D, hipStream_t stream, hipEvent_t e0, hipEvent_t e1) {
    const size_t lds = handleLdsBytes(hs.HW, hs.W, hs.CAP, hs.partial_obs, hs.bot_off != 0);
    dim3 grid((unsigned)hs.n_games), block(64);
    KDyn DH = D;  // a HELP instance's argument: the helper wave's area after the game's LDS
    DH.help_off = (int32_t)ldsAlign16(lds);
#define LAUNCH(kern, g_, b_, l_, s_, ...) hipExtLaunchKernelGGL(kern, g_, b_, (uint32_t)(l_), s_, e0, e1, 0, __VA_ARGS__)
#define ENV(...) LAUNCH((k_env<__VA_ARGS__>), grid, block, lds, stream, D.state, ds, D)
#define ENV_HELP(bytes, ...) LAUNCH((k_env<__VA_ARGS__>), grid, dim3(128), (size_t)DH.help_off + (bytes), stream, D.state, ds, DH)
    switch (envInstance(mode, hs, D)) {
        case EI_STEADY16: ENV(MODE_STEP, 16, 320, false, true, false, false, true); break;
        case EI_MULTI16: ENV(MODE_STEP, 16, 320, false, true); break;
        case EI_STEP16: ENV(MODE_STEP, 16, 320, false); break;
        case EI_HELP8: ENV_HELP(HELP8_LDS, MODE_STEP, 8, 128, false, true, true); break;
        case EI_MULTI8: ENV(MODE_STEP, 8, 128, false, true); break;
        case EI_STEP8: ENV(MODE_STEP, 8, 128, false); break;
        case EI_HELP32PO: ENV_HELP(HELP32PO_LDS, MODE_STEP, 32, 320, true, true, true); break;
        case EI_MULTI32PO: ENV(MODE_STEP, 32, 320, true, true); break;
        case EI_STEP32PO: ENV(MODE_STEP, 32, 320, true); break;
        case EI_STEP_LR: ENV(MODE_STEP, 0, 0, false, false, false, true); break;
        case EI_STEP: ENV(MODE_STEP, 0); break;
        case EI_RESET_LR: ENV(MODE_RESET, 0, 0, false, false, false, true); break;
        case EI_RESET: ENV(MODE_RESET, 0); break;
        case EI_PLAYOUT: ENV(MODE_PLAYOUT, 0); break;
        case EI_TRACE16: ENV(MODE_TRACE, 16, 320); break;
        case EI_TRACE8: ENV(MODE_TRACE, 8, 128); break;
        case EI_TRACE: ENV(MODE_TRACE, 0); break;
        case EI_MASKS: ENV(MODE_MASKS, 0); break;
    }
#undef ENV_HELP
#undef ENV
#undef LAUNCH
    return hipGetLastError();
}
// launchEnv(MODE_STEP) would run a specialised self-play kernel (16x16 / 8x8 full observability,
// 32x32 partially observable), the ones whose games can iterate several steps in one launch
// (KDyn.n_iter, MULTI instances): every shape of SPEC_SHAPES has one
bool envIterable(const KStatic& hs) { return specialisedShape(hs) >= 0; }

// The handle's LDS bytes, and the selection for a handle and a launch described by a few numbers: EnvInst, plus 256
// where envIterable holds.  A launch starts from the steady state's arguments (steadyDyn) and changes the fields
// named.  Not part of include/mrts.h: the tests' view of the host-side facts (tests/test_launch_facts_cpu.py).
extern "C" int mrts_internal_lds_probe(int HW, int W, int CAP, int po, int light_rush) {
    return (int)handleLdsBytes(HW, W, CAP, po, light_rush != 0);
}
extern "C" int mrts_internal_launch_probe(int H, int W, int CAP, int po, int K, int ntypes, int radius, int all_selfplay,
                                          int light_rush, int mode, int n_iter, int rows, int uniform, int masks, int obs) {
    KStatic hs{};
    hs.n_games = 512;
    hs.n_sp_games = all_selfplay ? 512 : 511;
    hs.utt.K = K;
    hs.utt.ntypes = ntypes;
    hs.utt.maxAttackRadius = radius;
    hs.H = H;
    hs.W = W;
    hs.HW = H * W;
    hs.CAP = CAP;
    hs.partial_obs = po;
    hs.bot_off = light_rush ? stateWords(CAP, H * W) : 0;
    void* const some = g_probeBuf;
    KDyn D = steadyDyn();
    D.n_iter = n_iter;
    D.rows = rows ? (const int32_t*)some : nullptr;
    D.uni_actions = uniform ? (int32_t*)some : nullptr;
    if (!masks) D.masks = nullptr;
    if (!obs) D.obs = nullptr;
    return (int)envInstance(mode, hs, D) | (envIterable(hs) ? 256 : 0);
}
}  // namespace mrts
