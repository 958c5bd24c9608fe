// mrts_host.cpp — host runtime behind include/mrts.h: the handle, per-game state allocation in HBM, kernel
// launches, the HIP and RCCL plumbing and the Java-compatible host-pointer API.  What needs no GPU (unit-type
// tables, map parsing, state JSON, the canonical dump, the checkpoint header, mrts_create's configuration half) is
// in mrts_hostdata.cpp.  Compiled by hipcc into microrts_amd/libmrts.so.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types only: the entry points are taken from the RCCL library the process loaded

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mrts.h"
#include "mrts_hostdata.h"
#include "mrts_internal.h"
#include "mrts_launch.h"

using namespace mrts;

static thread_local std::string g_err;

#define HIPCHK(x)                                                                         \
    do {                                                                                  \
        hipError_t e_ = (x);                                                              \
        if (e_ != hipSuccess) throw Fail{-EIO, std::string(#x) + ": " + hipGetErrorString(e_)}; \
    } while (0)

struct mrts_env : HandleConfig {
    hipStream_t stream = nullptr;
    size_t ldsNeed() const { return handleLdsBytes(HW, W, CAP, partialObs, hasLightRush != 0); }
    int32_t* d_state = nullptr;
    int32_t* d_tmpl = nullptr;
    int32_t* d_tmplOff = nullptr;
    int32_t* d_gameKind = nullptr;
    // library-owned buffers for the host-pointer API
    int32_t* d_actions = nullptr;
    int32_t* d_players = nullptr;
    int32_t* d_obs = nullptr;
    double* d_reward = nullptr;
    uint8_t* d_done = nullptr;
    uint8_t* d_masks = nullptr;
    int32_t* h_obs = nullptr;
    uint8_t* h_masks = nullptr;    // mrts_get_masks_host: pinned, library-owned (Java reuses its mask array)
    int32_t* h_masks32 = nullptr;  // mrts_get_masks_i32_host
    double* h_reward = nullptr;
    uint8_t* h_done = nullptr;
    std::vector<int32_t> h_stateScratch;

    KStatic hstatic;
    KStatic* d_static = nullptr;
    // persistent-buffer observations (mrts_set_obs_delta; partially observable views): the buffer the
    // last launch wrote observations to (null after a launch that changed the state without one, or
    // after an invalidation) and the per-game render records (PO handles on delta-capable maps)
    int obsDelta = 0;
    int16_t* obs16 = nullptr;  // mrts_set_obs16: int16 copy of each observation write (full observability)
    uint8_t* obs8 = nullptr;   // the exchange's uint8 transport (mrts_set_exchange_bytes(env, 1))
    int exBytes = 2;           // bytes per value of the exchanged observation: 2 (int16) or 1 (uint8)
    int multiStep = 1;  // mrts_rollout_fused_dev may run several steps per launch (mrts_set_multi_step)
    const int32_t* lastObsPtr = nullptr;
    int32_t* d_poPrev = nullptr;
    uint32_t* d_prioTab = nullptr;  // multi-step launches: per-SIMD issue-rank table (KDyn.prio_tab)
    int32_t* d_renderErr = nullptr; // the record renders' overflow flag (mrts_render_status)
    unsigned long long* d_packOverflow = nullptr;  // rows mrts_policy_head_pack_dev cut at cap (mrts_policy_head_pack_status)
    unsigned long long* d_obsPackCnt = nullptr;  // packed observation rows: lossy rows, bad reads (mrts_obs_packed_status)
    int32_t* d_bal = nullptr;       // multi-step launches: balanced game placement (KDyn.bal)
    bool exPending[2] = {false, false};  // exDone[b] was recorded by an earlier (eager) exchange call
    hipStream_t exLastStream = nullptr;  // the stream of the last eager exchange call (already waits for them)
    // native observation exchange (mrts_exchange_init): an RCCL communicator over this handle's ranks,
    // its own communication stream, and per send buffer the step-ready / collective-done events
    ncclComm_t exComm = nullptr;
    int exRanks = 0, exRank = 0;
    bool exLoop = false;  // mrts_exchange_init_loopback: the test transport (no RCCL), see exAllGather
    // compact observation records (mrts_set_records): units per record (0 = off), steps per launch of a
    // records rollout (0 = as many as a launch can run)
    int recUnits = 0, recSteps = 0;
    hipStream_t exStream = nullptr;
    hipEvent_t exReady[2] = {nullptr, nullptr}, exDone[2] = {nullptr, nullptr};
    // mrts_capture_begin / _end / mrts_replay: the calls enqueued in between, as one instantiated graph
    hipGraph_t capGraph = nullptr;
    hipGraphExec_t capExec = nullptr;
    int poWords = 0;
    // delta mask writes: which buffer / player the last mask write went to
    const uint8_t* lastMaskPtr = nullptr;
    int lastMaskPlayer = -1;
    uint32_t* d_source = nullptr;
    // delta policy writes: candidate set of the last source-form policy write, and where it went
    uint32_t* d_polPrev = nullptr;
    // Java row layout (mrts_step_rows*): accepted-pair scratch [n_games][n_rows][2] and host staging
    uint32_t* d_pairs = nullptr;
    int pairsRows = 0;
    int32_t* d_rowsStage = nullptr;
    size_t rowsStageInts = 0;
    int32_t* d_masks32 = nullptr;
    int32_t* d_copyPairs = nullptr;  // mrts_copy_games staging
    int copyPairsCap = 0;
    float* d_eval = nullptr;         // mrts_evaluate staging
    const int32_t* lastPolicyActions = nullptr;
    bool polValid = false;
    const int32_t* fusedActions = nullptr;  // buffer the last fused-policy step wrote (delta base), or null
    // mrts_set_rollout_events: HIP events the next native rollout records around its launches (one shot)
    hipEvent_t evStart = nullptr, evEnd = nullptr;
    mutable uint32_t launchStamp = 0;       // KDyn.fwd_stamp of the last k_env launch (never 0)
    // every step's Responses (mrts_set_step_responses): the ring and its capacity in steps; during a rollout
    // call respK = the call's next step index (each MODE_STEP launch writes its steps there and advances
    // it), -1 outside rollout calls
    double* respRew = nullptr;
    uint8_t* respDone = nullptr;
    int32_t respMax = 0;
    mutable int32_t respK = -1;
    int polParity = 0;
    // the kernels store observations and mask chunks as 16-byte vectors
    static void checkAlign(const KDyn& D) {
        if (((uintptr_t)D.obs & 15) || ((uintptr_t)D.masks & 15)) throw Fail{-EINVAL, "obs / masks buffers must be 16-byte aligned"};
        if (((uintptr_t)D.reward & 7) || ((uintptr_t)D.actions & 3) || ((uintptr_t)D.rows & 3) || ((uintptr_t)D.players & 3))
            throw Fail{-EINVAL, "misaligned buffer"};
    }
    // every launch that changes the state or writes observations; the library-owned buffer of the
    // host-pointer API is always persistent
    void prepObs(KDyn& D) {
        D.obs16 = D.obs ? obs16 : nullptr;
        D.obs8 = D.obs ? obs8 : nullptr;
        D.obs_delta = (D.obs && D.obs == lastObsPtr && (obsDelta || D.obs == d_obs)) ? 1 : 0;
        D.po_prev = D.obs ? d_poPrev : nullptr;
        D.po_words = poWords;
        lastObsPtr = D.obs;
    }
    void prepMasks(KDyn& D) {
        checkAlign(D);
        D.source = D.masks ? d_source : nullptr;
        D.mask_delta = (maskDelta && D.masks && D.masks == lastMaskPtr && D.mask_player == lastMaskPlayer) ? 1 : 0;
        if (D.masks) {
            lastMaskPtr = D.masks;
            lastMaskPlayer = D.mask_player;
        }
    }
    // launch arguments with nothing set (the launches that take no caller buffers fill in their few fields)
    static KDyn noArgs() {
        KDyn D;
        std::memset(&D, 0, sizeof(D));
        return D;
    }
    // The arguments of a reset or step launch from the caller's buffers (grid actions or Java rows, either may be
    // null), with the mask and observation writes' delta bookkeeping done (prepMasks, then prepObs).  What only one
    // path sets (fused policy or uniform fields, n_rows, n_iter, records) is added by that path.
    KDyn launchArgs(const int32_t* actions, const int32_t* rows, const int32_t* players, int32_t* obs, double* reward,
                    uint8_t* done, uint8_t* masks, int32_t mask_player) {
        KDyn D = noArgs();
        D.actions = actions;
        D.rows = rows;
        D.players = players;
        D.obs = obs;
        D.reward = reward;
        D.done = done;
        D.masks = masks;
        D.mask_player = mask_player;
        prepMasks(D);
        prepObs(D);
        return D;
    }
    // the state changed behind the kernels' backs (an injected state, a restore): the next mask, observation and
    // policy writes are full ones
    void invalidateWrites() {
        lastMaskPtr = nullptr;
        lastObsPtr = nullptr;
        polValid = false;
        fusedActions = nullptr;
    }
    void buildStatic() {
        std::memset(&hstatic, 0, sizeof(hstatic));
        hstatic.utt = utt;
        hstatic.H = H;
        hstatic.W = W;
        hstatic.HW = HW;
        hstatic.CAP = CAP;
        hstatic.n_games = nGames;
        hstatic.n_sp_games = nSpGames;
        hstatic.n_rewards = (int32_t)rewardKinds.size();
        hstatic.reward_need = 0;
        for (size_t j = 0; j < rewardKinds.size(); j++) {
            const int k = rewardKinds[j];
            hstatic.reward_kinds[j] = k;
            if (k >= RF_RESOURCE_GATHER && k <= RF_PRODUCE_COMBAT_UNIT) hstatic.reward_need |= RN_COUNTS;
            if (k == RF_RESOURCE_GATHER) hstatic.reward_need |= RN_RESOURCES;
            if (k == RF_CLOSER_TO_ENEMY_BASE || k == RF_CLOSER_TO_ENEMY_UNIT) hstatic.reward_need |= RN_CLOSER;
        }
        hstatic.max_steps = maxSteps;
        hstatic.C = C;
        hstatic.partial_obs = partialObs;
        hstatic.state = d_state;
        hstatic.tmpl = d_tmpl;
        hstatic.tmpl_off = d_tmplOff;
        hstatic.game_kind = d_gameKind;
        hstatic.bot_off = hasLightRush ? stateWords(CAP, HW) : 0;
        hstatic.bot_lds = hasLightRush ? (int32_t)ldsLightRushOff(HW, W, CAP, partialObs) : 0;
        hstatic.bot_types = botTypes;
    }
    hipError_t launch(int mode, const KDyn& Din, hipStream_t s, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr) const {
        KDyn D = Din;
        D.state = d_state;
        D.state_words = (int32_t)blockWords();
        D.H = H;
        D.W = W;
        D.HW = HW;
        D.CAP = CAP;
        D.n_sp_games = nSpGames;
        D.n_rewards = hstatic.n_rewards;
        D.max_steps = hstatic.max_steps;
        D.C = hstatic.C;
        D.reward_need = hstatic.reward_need;
        D.reward_kinds4 = 0;
        for (int j = 0; j < hstatic.n_rewards; j++) D.reward_kinds4 |= (uint32_t)hstatic.reward_kinds[j] << (4 * j);
        if (++launchStamp == 0) ++launchStamp;  // H_FWD = 0 means "no forwarded rows"
        D.fwd_stamp = launchStamp;
        D.prio_tab = D.n_iter > 1 ? d_prioTab : nullptr;
        D.bal = D.n_iter > 1 ? d_bal : nullptr;
        D.obs_img = obsImg;
        if (mode == MODE_STEP && respK >= 0 && respRew) {  // the call's Responses ring (RespScope)
            const size_t stride = (size_t)nSlots * hstatic.n_rewards;
            D.reward = respRew + (size_t)respK * stride;
            D.done = respDone + (size_t)respK * stride;
            D.resp_stride = (int32_t)stride;
            respK += D.n_iter > 1 ? D.n_iter : 1;
        }
        return launchEnv(mode, hstatic, d_static, D, s, e0, e1);
    }
    // a state block about to be injected: if any live unit's hp or resources leaves 0..255, the byte
    // renders (KDyn.obs_img, the uint8 exchange transport) can no longer show it — turn them off for
    // good (300 would have rendered as 44, -5 as 251)
    void noteValues(const int32_t* s) {
        if (!valuesFitBytes(s, CAP)) obsImg = 0;
    }
    int gameOfSlot(int slot, int* player) const {
        if (slot < 2 * nSpGames) {
            *player = slot & 1;
            return slot / 2;
        }
        *player = 0;
        return nSpGames + (slot - 2 * nSpGames);
    }
};

namespace {

// Every entry point that returns an error code runs its body through one of these two (guardCall,
// mrts_hostdata.h): a refusal's text goes to mrts_last_error(), a null handle is -EINVAL "null handle".
template <class F>
int guardedCall(F&& body) {
    return guardCall(g_err, body);
}
template <class F>
int guarded(const mrts_env* env, F&& body) {
    return guardCall(g_err, [&] {
        if (!env) throw Fail{-EINVAL, "null handle"};
        return body();
    });
}

hipStream_t pickStream(mrts_env*, void* s) { return (hipStream_t)s; }  // NULL = HIP's default stream, like every HIP API

void checkFlagsAfter(mrts_env* env) {  // Java exceptions → error codes
    std::vector<uint32_t> fl((size_t)env->nSlots);
    mrts_error_flags(env, fl.data());
    uint32_t all = 0;
    for (auto f : fl) all |= f;
    if (all & (MRTS_ERR_PRODUCE_TYPE)) throw Fail{-EINVAL, "decoded produce type out of range (Java: IndexOutOfBoundsException)"};
    if (all & (MRTS_ERR_CAPACITY)) throw Fail{-ENOSPC, "unit capacity exhausted"};
    if (all & (MRTS_ERR_ADDUNIT | MRTS_ERR_MOVE_COLLISION)) throw Fail{-EFAULT, "two units in one position (Java: addUnit exception)"};
}

}  // namespace

extern "C" {

const char* mrts_last_error(void) { return g_err.c_str(); }

int mrts_create(const mrts_config* cfg, mrts_env** out) {
    mrts_env* env = nullptr;
    const int r = guardedCall([&] {
        if (!cfg || !out) throw Fail{-EINVAL, "null argument"};
        const CreatePlan P = planCreate(cfg);  // host-only validation (testable without a GPU); device work starts below
        env = new mrts_env();
        static_cast<HandleConfig&>(*env) = P.cfg;
        HIPCHK(hipSetDevice(cfg->device));
        HIPCHK(hipStreamCreateWithFlags(&env->stream, hipStreamNonBlocking));
        hipDeviceProp_t prop;
        HIPCHK(hipGetDeviceProperties(&prop, cfg->device));
        const size_t lds = env->ldsNeed();
        if (lds > 160 * 1024) throw Fail{-EINVAL, "map too large for LDS"};
        if (lds > 64 * 1024) HIPCHK(prepareLds(lds));
        if (P.mostMapUnits > env->maxUnits) throw Fail{-ENOSPC, "a map holds more units than max_units"};
        const size_t sw = env->blockWords();
        HIPCHK(hipMalloc(&env->d_state, sw * env->nGames * 4));
        if (env->partialObs && poDeltaShape(env->H, env->W)) {  // PO render records (delta observations)
            env->poWords = poPrevWords(env->CAP, env->H, env->HW);
            HIPCHK(hipMalloc(&env->d_poPrev, (size_t)env->poWords * env->nGames * 4));
            HIPCHK(hipMemset(env->d_poPrev, 0, (size_t)env->poWords * env->nGames * 4));
        }
        HIPCHK(hipMalloc(&env->d_tmpl, P.blob.size() * 4));
        HIPCHK(hipMalloc(&env->d_tmplOff, (size_t)env->nGames * 4));
        HIPCHK(hipMalloc(&env->d_gameKind, (size_t)env->nGames * 4));
        HIPCHK(hipMemcpy(env->d_tmpl, P.blob.data(), P.blob.size() * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(env->d_tmplOff, env->tmplOffHost.data(), (size_t)env->nGames * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(env->d_gameKind, env->gameKindHost.data(), (size_t)env->nGames * 4, hipMemcpyHostToDevice));
        // headers: the random streams' seeds, the rest zero
        static_assert(H_RNG_DAMAGE == H_RNG_CANCEL + 2 && H_RNG_SAMPLER == H_RNG_CANCEL + 4, "CreatePlan::rngWords");
        std::vector<int32_t> hdr(sw * env->nGames, 0);
        for (int g = 0; g < env->nGames; g++) std::memcpy(&hdr[(size_t)g * sw + H_RNG_CANCEL], &P.rngWords[(size_t)6 * g], 6 * 4);
        HIPCHK(hipMemcpy(env->d_state, hdr.data(), hdr.size() * 4, hipMemcpyHostToDevice));
        // host-API buffers
        const size_t S = (size_t)env->nSlots;
        HIPCHK(hipMalloc(&env->d_actions, S * env->HW * 7 * 4));
        HIPCHK(hipMalloc(&env->d_players, S * 4));
        HIPCHK(hipMalloc(&env->d_obs, S * env->C * env->HW * 4));
        const size_t R = env->rewardKinds.size();
        HIPCHK(hipMalloc(&env->d_reward, S * R * 8));
        HIPCHK(hipMalloc(&env->d_done, S * R));
        HIPCHK(hipMalloc(&env->d_masks, S * env->HW * env->K));
        HIPCHK(hipHostMalloc(&env->h_obs, S * env->C * env->HW * 4, hipHostMallocDefault));
        HIPCHK(hipHostMalloc(&env->h_reward, S * R * 8, hipHostMallocDefault));
        HIPCHK(hipHostMalloc(&env->h_done, S * R, hipHostMallocDefault));
        HIPCHK(hipMemset(env->d_players, 0, S * 4));
        // the Java clients' arrays start as zeros (new double[rfs.length], JNIGridnetClientSelfPlay.java:
        // 134-135); a self-play reset leaves slots >= 2 alone, so they must not start as garbage
        HIPCHK(hipMemset(env->d_reward, 0, S * R * 8));
        HIPCHK(hipMemset(env->d_done, 0, S * R));
        // static kernel parameters → device buffer
        env->buildStatic();
        HIPCHK(hipMalloc(&env->d_static, sizeof(KStatic)));
        HIPCHK(hipMemcpy(env->d_static, &env->hstatic, sizeof(KStatic), hipMemcpyHostToDevice));
        if (envIterable(env->hstatic)) {  // entries carry a launch stamp: stale ones are ignored, zero = empty
            HIPCHK(hipMalloc(&env->d_prioTab, (size_t)PRIO_KEYS * 16 * 4));
            HIPCHK(hipMemset(env->d_prioTab, 0, (size_t)PRIO_KEYS * 16 * 4));
            HIPCHK(hipMalloc(&env->d_bal, ((size_t)BAL_COST + 2 * (size_t)env->nGames) * 4));
            // header and costs zero, the permutation the identity: a class slice no launch rewrote stays a
            // permutation of its games (balancePerm writes each XCD class's slice on its own)
            std::vector<int32_t> bal((size_t)BAL_COST + 2 * (size_t)env->nGames, 0);
            for (int g = 0; g < env->nGames; g++) bal[(size_t)BAL_COST + env->nGames + g] = g;
            HIPCHK(hipMemcpy(env->d_bal, bal.data(), bal.size() * 4, hipMemcpyHostToDevice));
        }
        // initial state = reset (the Java constructor loads the maps)
        KDyn D = mrts_env::noArgs();
        D.players = env->d_players;
        HIPCHK(env->launch(MODE_RESET, D, env->stream));
        HIPCHK(hipStreamSynchronize(env->stream));
        *out = env;
        return 0;
    });
    if (r && env) mrts_destroy(env);
    return r;
}

int mrts_dims(const mrts_env* env, int32_t* n_slots, int32_t* H, int32_t* W, int32_t* C, int32_t* K) {
    if (!env) return -EINVAL;
    if (n_slots) *n_slots = env->nSlots;
    if (H) *H = env->H;
    if (W) *W = env->W;
    if (C) *C = env->C;
    if (K) *K = env->K;
    return 0;
}

void* mrts_stream(mrts_env* env) { return env ? (void*)env->stream : nullptr; }

int mrts_reset_dev(mrts_env* env, const int32_t* d_players, int32_t* d_obs, double* d_reward, uint8_t* d_done,
                   uint8_t* d_masks, int32_t mask_player, void* stream) {
    return guarded(env, [&] {
        HIPCHK(hipSetDevice(env->device));
        const KDyn D = env->launchArgs(nullptr, nullptr, d_players, d_obs, d_reward, d_done, d_masks, mask_player);
        env->fusedActions = nullptr;
        HIPCHK(env->launch(MODE_RESET, D, pickStream(env, stream)));
        return 0;
    });
}

int mrts_step_dev(mrts_env* env, const int32_t* d_actions, const int32_t* d_players, int32_t* d_obs, double* d_reward,
                  uint8_t* d_done, uint8_t* d_masks, int32_t mask_player, void* stream) {
    return guarded(env, [&] {
        if (env->forwardModel) throw Fail{-EINVAL, "a forward-model handle advances through mrts_playout*"};
        if (!d_actions) throw Fail{-EINVAL, "actions is null"};
        HIPCHK(hipSetDevice(env->device));
        const KDyn D = env->launchArgs(d_actions, nullptr, d_players, d_obs, d_reward, d_done, d_masks, mask_player);
        if (d_masks || d_actions == env->fusedActions) env->fusedActions = nullptr;
        HIPCHK(env->launch(MODE_STEP, D, pickStream(env, stream)));
        return 0;
    });
}

namespace {
// records rollout (mrts_rollout_*_records_dev): the launch writes its steps' records into `chunk`, the
// part of the receive buffer one all-gather fills, at this rank's place ([rank][steps][games][words]):
// the chunk holds `steps` steps, and this launch's first one is step `first` of them
struct RecPlan {
    uint32_t* chunk;
    int rank;
    int steps, first;
};
void planRecords(const mrts_env* env, KDyn& D, const RecPlan* rec) {
    if (!rec) return;
    D.rec_units = env->recUnits;
    D.rec_out = rec->chunk + ((size_t)rec->rank * rec->steps + rec->first) * env->nGames * recWords(env->recUnits, env->partialObs);
}
// n_iter consecutive fused steps (next_step, next_step + 1, ...) as ONE launch when the handle runs a
// specialised full-observability self-play kernel and is in the steady fused state (the previous
// launch was a fused step on these buffers: delta masks and policy rows, forwarded action words);
// else one step.  Returns the number of steps enqueued.
int stepFused(mrts_env* env, int32_t* d_actions, const int32_t* d_players, int32_t* d_obs, double* d_reward, uint8_t* d_done,
              uint8_t* d_masks, int32_t mask_player, uint64_t seed, uint32_t next_step, int32_t n_iter, void* stream,
              hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr, const RecPlan* rec = nullptr) {
    if (!d_actions || !d_masks) throw Fail{-EINVAL, "actions and masks are required"};
    if (env->forwardModel) throw Fail{-EINVAL, "a forward-model handle advances through mrts_playout*"};
    HIPCHK(hipSetDevice(env->device));
    KDyn D = env->launchArgs(d_actions, nullptr, d_players, d_obs, d_reward, d_done, d_masks, mask_player);
    D.pol_actions = d_actions;
    D.pol_seed = seed;
    D.pol_step = next_step;
    D.pol_slot_base = env->slotIdBase;
    D.pol_delta = (D.mask_delta && env->fusedActions == d_actions) ? 1 : 0;
    D.fwd_read = env->fusedActions == d_actions ? 1 : 0;  // games check H_FWD == this stamp - 1
    const bool steady = D.pol_delta && D.fwd_read && D.mask_delta && envIterable(env->hstatic);
    D.n_iter = (steady && n_iter > 1) ? n_iter : 1;
    planRecords(env, D, rec);
    HIPCHK(env->launch(MODE_STEP, D, pickStream(env, stream), e0, e1));
    env->fusedActions = d_actions;
    if (env->lastPolicyActions == d_actions) env->polValid = false;  // the standalone policy's delta base is stale
    return D.n_iter;
}
}  // namespace

int mrts_step_fused_dev(mrts_env* env, int32_t* d_actions, const int32_t* d_players, int32_t* d_obs, double* d_reward,
                        uint8_t* d_done, uint8_t* d_masks, int32_t mask_player, uint64_t seed, uint32_t next_step,
                        void* stream) {
    return guarded(env, [&] {
        stepFused(env, d_actions, d_players, d_obs, d_reward, d_done, d_masks, mask_player, seed, next_step, 1, stream);
        return 0;
    });
}

namespace {
// the one-shot rollout events (mrts_set_rollout_events): recorded on the rollout's stream right
// before its first launch / right after its last, then forgotten
struct RolloutEvents {
    mrts_env* env;
    hipStream_t s;
    hipEvent_t end = nullptr;
    RolloutEvents(mrts_env* e, void* stream) : env(e), s(pickStream(e, stream)) {
        if (env->evStart) HIPCHK(hipEventRecord(env->evStart, s));
        end = env->evEnd;
        env->evStart = env->evEnd = nullptr;
    }
    void done() {
        if (end) HIPCHK(hipEventRecord(end, s));
    }
};
}  // namespace

namespace {
// a rollout call's span of the Responses ring (mrts_set_step_responses): the step launches write step k
// of the call at ring step k instead of d_reward / d_done (launch() points them at the ring; the last
// step's are ring step n_steps - 1 — no copy back, which cost a with_gather window ~5 %)
struct RespScope {
    mrts_env* env;
    RespScope(mrts_env* e, int32_t n_steps) : env(e) {
        if (n_steps < 0) throw Fail{-EINVAL, "bad rollout arguments"};
        if (!env->respRew) return;
        if (n_steps > env->respMax) throw Fail{-EINVAL, "more steps than the Responses ring holds (mrts_set_step_responses)"};
        env->respK = 0;
    }
    ~RespScope() { env->respK = -1; }
};
}  // namespace

int mrts_set_step_responses(mrts_env* env, double* d_rewards, uint8_t* d_dones, int32_t max_steps) {
    return guarded(env, [&] {
        if (!d_rewards != !d_dones || (d_rewards && max_steps < 1)) throw Fail{-EINVAL, "both rings and max_steps >= 1, or both NULL"};
        // the kernel forms a ring step's offset as a 32-bit product (it x n_slots x n_rewards)
        if (d_rewards && (uint64_t)max_steps * (uint64_t)env->nSlots * (uint64_t)env->hstatic.n_rewards >= (1ull << 32))
            throw Fail{-EINVAL, "the Responses ring exceeds 2^32 entries"};
        env->respRew = d_rewards;
        env->respDone = d_dones;
        env->respMax = d_rewards ? max_steps : 0;
        return 0;
    });
}

int mrts_set_rollout_events(mrts_env* env, void* start, void* end) {
    return guarded(env, [&] {
        env->evStart = (hipEvent_t)start;
        env->evEnd = (hipEvent_t)end;
        return 0;
    });
}

int mrts_rollout_fused_dev(mrts_env* env, int32_t* d_actions, const int32_t* d_players, int32_t* d_obs, double* d_reward,
                           uint8_t* d_done, uint8_t* d_masks, int32_t mask_player, uint64_t seed, uint32_t first_next_step,
                           int32_t n_steps, void* stream) {
    return guarded(env, [&] {
        // the timing events ride on the launches: start with the first, end re-recorded by each (the last wins)
        RespScope rs(env, n_steps);
        hipEvent_t e0 = env->evStart, e1 = env->evEnd;
        env->evStart = env->evEnd = nullptr;
        if (n_steps == 0) {
            RolloutEvents ev(env, stream);
            ev.done();
        }
        for (int32_t k = 0; k < n_steps;) {
            const int32_t n = std::min<int32_t>(n_steps - k, env->multiStep ? MRTS_MAX_ITER : 1);
            k += stepFused(env, d_actions, d_players, d_obs, d_reward, d_done, d_masks, mask_player, seed,
                           first_next_step + (uint32_t)k, n, stream, e0, e1);
            e0 = nullptr;
        }
        return 0;
    });
}

int mrts_set_multi_step(mrts_env* env, int32_t on) {
    return guarded(env, [&] {
        env->multiStep = on ? 1 : 0;
        return 0;
    });
}

int mrts_multi_step_capable(const mrts_env* env) { return (env && env->multiStep && envIterable(env->hstatic)) ? 1 : 0; }

int mrts_step_rows_dev(mrts_env* env, const int32_t* d_rows, int32_t n_rows, const int32_t* d_players, int32_t* d_obs,
                       double* d_reward, uint8_t* d_done, uint8_t* d_masks, int32_t mask_player, void* stream) {
    return guarded(env, [&] {
        if (env->forwardModel) throw Fail{-EINVAL, "a forward-model handle advances through mrts_playout*"};
        if (!d_rows && n_rows > 0) throw Fail{-EINVAL, "rows is null"};
        if (n_rows < 0 || (size_t)n_rows * env->nSlots * 8 >= ((size_t)1 << 31)) throw Fail{-EINVAL, "bad n_rows"};
        HIPCHK(hipSetDevice(env->device));
        if (n_rows > env->pairsRows) {
            hipStream_t s = pickStream(env, stream);
            HIPCHK(hipStreamSynchronize(s));  // the old scratch may still be in use on the stream
            (void)hipFree(env->d_pairs);
            env->d_pairs = nullptr;
            HIPCHK(hipMalloc(&env->d_pairs, (size_t)env->nGames * n_rows * 2 * 4));
            env->pairsRows = n_rows;
        }
        KDyn D = env->launchArgs(nullptr, d_rows, d_players, d_obs, d_reward, d_done, d_masks, mask_player);
        D.n_rows = n_rows;
        D.pairs = env->d_pairs;
        if (d_masks) env->fusedActions = nullptr;
        HIPCHK(env->launch(MODE_STEP, D, pickStream(env, stream)));
        return 0;
    });
}

int mrts_get_masks_i32_dev(mrts_env* env, int32_t player, int32_t* d_out, void* stream) {
    return guarded(env, [&] {
        if (!d_out) throw Fail{-EINVAL, "out is null"};
        int r = mrts_get_masks_dev(env, player, env->d_masks, stream);
        if (r) return r;
        HIPCHK(launchWiden(env->d_masks, d_out, (size_t)env->nSlots * env->HW * env->K, pickStream(env, stream)));
        return 0;
    });
}

int mrts_onehot_features(const mrts_env* env) {
    const int base = 5 + 5 + 3 + (env->utt.ntypes + 1) + 6 + 2;
    return base + 2 * (env->C - 6);
}

int mrts_onehot_dev(mrts_env* env, const int32_t* d_obs, uint8_t* d_out, void* stream) {
    return guarded(env, [&] {
        if (!d_obs || !d_out) throw Fail{-EINVAL, "null buffer"};
        HIPCHK(hipSetDevice(env->device));
        HIPCHK(launchOneHot(d_obs, d_out, env->nSlots, env->HW, env->C, env->utt.ntypes, pickStream(env, stream)));
        return 0;
    });
}

int mrts_get_masks_dev(mrts_env* env, int32_t player, uint8_t* d_out, void* stream) {
    return guarded(env, [&] {
        if (!d_out) throw Fail{-EINVAL, "out is null"};
        HIPCHK(hipSetDevice(env->device));
        KDyn D = mrts_env::noArgs();  // no observation write: lastObsPtr stays
        D.masks = d_out;
        D.mask_player = player;
        D.players = env->d_players;
        env->prepMasks(D);
        env->fusedActions = nullptr;
        HIPCHK(env->launch(MODE_MASKS, D, pickStream(env, stream)));
        return 0;
    });
}

int mrts_policy_uniform_dev(mrts_env* env, uint64_t seed, uint32_t step, int32_t* d_actions, void* stream) {
    return guarded(env, [&] {
        if (!d_actions) throw Fail{-EINVAL, "null argument"};
        if ((uintptr_t)d_actions & 3) throw Fail{-EINVAL, "misaligned buffer"};
        HIPCHK(hipSetDevice(env->device));
        HIPCHK(launchPolicyUniform(d_actions, env->nSlots, env->HW, env->utt.ntypes, env->K - 23 - env->utt.ntypes, seed, step,
                                   (uint32_t)env->slotIdBase, pickStream(env, stream)));
        // the tensor no longer holds what a masked policy or a fused step wrote there
        if (env->fusedActions == d_actions) env->fusedActions = nullptr;
        if (env->lastPolicyActions == d_actions) env->polValid = false;
        return 0;
    });
}

namespace {
// n_iter fused uniform steps (step, step + 1, ...) as ONE launch on the multi-step shapes (the rows
// are drawn in the kernel, so no steady state is needed), else one.  Returns the steps enqueued.
int stepUniform(mrts_env* env, int32_t* d_actions, const int32_t* d_players, int32_t* d_obs, double* d_reward, uint8_t* d_done,
                uint8_t* d_masks, int32_t mask_player, uint64_t seed, uint32_t step, int32_t n_iter, void* stream,
                hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr, const RecPlan* rec = nullptr) {
    if (!d_actions) throw Fail{-EINVAL, "null argument"};
    if ((uintptr_t)d_actions & 3) throw Fail{-EINVAL, "misaligned buffer"};
    if (env->forwardModel) throw Fail{-EINVAL, "a forward-model handle advances through mrts_playout*"};
    HIPCHK(hipSetDevice(env->device));
    KDyn D = env->launchArgs(d_actions, nullptr, d_players, d_obs, d_reward, d_done, d_masks, mask_player);
    D.uni_actions = d_actions;
    D.uni_seed = seed;
    D.uni_step = step;
    D.uni_slot_base = (uint32_t)env->slotIdBase;
    // masks in a loop need the delta row sets of the previous write (kept in LDS between iterations)
    const bool loopable = envIterable(env->hstatic) && (!d_masks || D.mask_delta);
    D.n_iter = (loopable && n_iter > 1) ? n_iter : 1;
    planRecords(env, D, rec);
    if (d_masks || env->fusedActions == d_actions) env->fusedActions = nullptr;
    if (env->lastPolicyActions == d_actions) env->polValid = false;
    HIPCHK(env->launch(MODE_STEP, D, pickStream(env, stream), e0, e1));
    return D.n_iter;
}
}  // namespace

int mrts_step_uniform_dev(mrts_env* env, int32_t* d_actions, const int32_t* d_players, int32_t* d_obs, double* d_reward,
                          uint8_t* d_done, uint8_t* d_masks, int32_t mask_player, uint64_t seed, uint32_t step, void* stream) {
    return guarded(env, [&] {
        stepUniform(env, d_actions, d_players, d_obs, d_reward, d_done, d_masks, mask_player, seed, step, 1, stream);
        return 0;
    });
}

int mrts_rollout_uniform_dev(mrts_env* env, int32_t* d_actions, const int32_t* d_players, int32_t* d_obs, double* d_reward,
                             uint8_t* d_done, uint64_t seed, uint32_t first_step, int32_t n_steps, int32_t fused,
                             void* stream) {
    return guarded(env, [&] {
        RespScope rs(env, n_steps);
        if (fused) {
            hipEvent_t e0 = env->evStart, e1 = env->evEnd;  // on the launches (see mrts_rollout_fused_dev)
            env->evStart = env->evEnd = nullptr;
            for (int32_t k = 0; k < n_steps;) {
                const int32_t n = std::min<int32_t>(n_steps - k, env->multiStep ? MRTS_MAX_ITER : 1);
                k += stepUniform(env, d_actions, d_players, d_obs, d_reward, d_done, nullptr, 0, seed, first_step + (uint32_t)k, n,
                                 stream, e0, e1);
                e0 = nullptr;
            }
            return 0;
        }
        for (int32_t k = 0; k < n_steps; k++) {
            int r = mrts_policy_uniform_dev(env, seed, first_step + (uint32_t)k, d_actions, stream);
            if (!r) r = mrts_step_dev(env, d_actions, d_players, d_obs, d_reward, d_done, nullptr, 0, stream);
            if (r) return r;
        }
        return 0;
    });
}

}  // extern "C" (the exchange loop below is a template)
namespace {
// RCCL entry points, resolved by dlopen / dlsym from the library path the caller names (the one its
// process group already loaded: one RCCL instance per process)
struct Rccl {
    ncclResult_t (*getUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*commInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*allGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*commDestroy)(ncclComm_t) = nullptr;
    const char* (*errorString)(ncclResult_t) = nullptr;
};
Rccl g_rccl;
void loadRccl(const char* path) {
    if (g_rccl.allGather) return;
    void* h = dlopen(path && *path ? path : "librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) throw Fail{-ENOENT, std::string("cannot load RCCL: ") + dlerror()};
    Rccl r;
    r.getUniqueId = (decltype(r.getUniqueId))dlsym(h, "ncclGetUniqueId");
    r.commInitRank = (decltype(r.commInitRank))dlsym(h, "ncclCommInitRank");
    r.allGather = (decltype(r.allGather))dlsym(h, "ncclAllGather");
    r.commDestroy = (decltype(r.commDestroy))dlsym(h, "ncclCommDestroy");
    r.errorString = (decltype(r.errorString))dlsym(h, "ncclGetErrorString");
    if (!r.getUniqueId || !r.commInitRank || !r.allGather || !r.commDestroy || !r.errorString)
        throw Fail{-ENOENT, "the RCCL library lacks an entry point"};
    g_rccl = r;
}
void ncclChk(ncclResult_t r, const char* what) {
    if (r != ncclSuccess) throw Fail{-EIO, std::string(what) + ": " + g_rccl.errorString(r)};
}
bool exInited(const mrts_env* env) { return env->exComm != nullptr || env->exLoop; }
// The all-gather of `bytes` per rank from send into recv ([ranks][bytes]) on the exchange stream.  The
// loopback test transport (mrts_exchange_init_loopback) stands in for ranks - 1 peers whose data differ
// from this rank's: the bytes are blocks of `rows` rows of `rowBytes` (a step's games, or
// slots), and peer r's place receives this rank's blocks with the rows rotated by r - rank — peer r's row
// i is this rank's row (i + r - rank) mod rows — while this rank's own place is left as written.  So a
// wrong rank offset, stride or chunk base, or a render that reads another rank's place, shows on one GPU
// as a rotated (wrong) observation, not as a copy of the right one.
void exAllGather(mrts_env* env, const void* send, void* recv, size_t bytes, size_t rowBytes, size_t rows) {
    if (env->exLoop) {
        const size_t blk = rowBytes * rows, nblk = blk ? bytes / blk : 0;
        if (!blk || nblk * blk != bytes) throw Fail{-EINVAL, "loopback exchange: bytes are not whole blocks"};
        for (int r = 0; r < env->exRanks; r++) {
            uint8_t* dst = (uint8_t*)recv + (size_t)r * bytes;
            if (dst == send) continue;
            const size_t d = (size_t)(((r - env->exRank) % (int)rows + (int)rows) % (int)rows);  // rotation in rows
            const uint8_t* src = (const uint8_t*)send;
            // dst rows [0, rows - d) <- src rows [d, rows); dst rows [rows - d, rows) <- src rows [0, d), every block
            if (rows - d)
                HIPCHK(hipMemcpy2DAsync(dst, blk, src + d * rowBytes, blk, (rows - d) * rowBytes, nblk, hipMemcpyDeviceToDevice,
                                        env->exStream));
            if (d)
                HIPCHK(hipMemcpy2DAsync(dst + (rows - d) * rowBytes, blk, src, blk, d * rowBytes, nblk, hipMemcpyDeviceToDevice,
                                        env->exStream));
        }
        return;
    }
    ncclChk(g_rccl.allGather(send, recv, bytes, ncclUint8, env->exComm, env->exStream), "ncclAllGather");
}
// per step: wait until the collective that last read send buffer k % 2 is done, run the step (it
// writes its int16 observation there), then all-gather it into recv on the exchange stream
template <class StepFn>
void exchangeLoop(mrts_env* env, int32_t n_steps, const int32_t* d_obs, int16_t* d_send0, int16_t* d_send1, int16_t* d_recv,
                  void* stream, StepFn step) {
    if (!exInited(env)) throw Fail{-EINVAL, "mrts_exchange_init first"};
    // the step kernel writes the transport as part of its observation write (prepObs)
    if (!d_obs) throw Fail{-EINVAL, "the exchange needs an observation buffer (d_obs)"};
    if (env->exBytes == 1 && !env->obsImg) throw Fail{-ENOTSUP, "uint8 exchange: an observation value no longer fits a byte"};
    if (env->partialObs) throw Fail{-ENOTSUP, "the int16 transport is written for full observability only"};
    if (!d_send0 || !d_send1 || !d_recv || (((uintptr_t)d_send0 | (uintptr_t)d_send1) & 7))
        throw Fail{-EINVAL, "send buffers must be 8-byte aligned, recv non-null"};
    HIPCHK(hipSetDevice(env->device));
    hipStream_t s = pickStream(env, stream);
    int16_t* send[2] = {d_send0, d_send1};
    const bool u8 = env->exBytes == 1;  // the buffers then hold uint8 values (mrts_set_exchange_bytes)
    const size_t bytes = (size_t)env->nSlots * env->C * env->HW * (u8 ? 1 : 2);
    bool pending[2] = {false, false};
    int16_t* const saved = env->obs16;
    // a send buffer an earlier call's collective may still read: that call ended with its own stream
    // waiting for its collectives, so only a call on another stream waits for them here.  Not while
    // capturing: the events were recorded outside the capture, so the graph could not hold
    // that dependency — whoever replays a captured exchange orders it after the eager calls itself.
    hipStreamCaptureStatus cst = hipStreamCaptureStatusNone;
    HIPCHK(hipStreamIsCapturing(s, &cst));
    const bool capturing = cst != hipStreamCaptureStatusNone;
    for (int b = 0; b < 2; b++)
        if (env->exPending[b] && !capturing && s != env->exLastStream) HIPCHK(hipStreamWaitEvent(s, env->exDone[b], 0));
    try {
        for (int32_t k = 0; k < n_steps; k++) {
            const int b = k & 1;
            if (pending[b]) HIPCHK(hipStreamWaitEvent(s, env->exDone[b], 0));
            if (u8) env->obs8 = (uint8_t*)send[b];
            else env->obs16 = send[b];
            step(k);
            HIPCHK(hipEventRecord(env->exReady[b], s));
            HIPCHK(hipStreamWaitEvent(env->exStream, env->exReady[b], 0));
            exAllGather(env, send[b], d_recv, bytes, bytes / env->nSlots, env->nSlots);  // (loopback: rotate slots)
            HIPCHK(hipEventRecord(env->exDone[b], env->exStream));
            pending[b] = true;
            if (!capturing) env->exPending[b] = true;  // (a captured record is the graph's, not an eager event)
        }
        for (int b = 0; b < 2; b++)  // the caller's stream covers every collective of the call
            if (pending[b]) HIPCHK(hipStreamWaitEvent(s, env->exDone[b], 0));
        if (!capturing && n_steps > 0) env->exLastStream = s;
    } catch (...) {
        env->obs16 = saved;
        env->obs8 = nullptr;
        throw;
    }
    env->obs16 = saved;
    env->obs8 = nullptr;
}
// The compact-record exchange (mrts_rollout_*_records_dev): every step's game records go into the receive
// buffer at this rank's place of its chunk; after each chunk, an in-place all-gather of it on the exchange
// stream (it overlaps the next chunk's launch).  step(k, n, plan) enqueues up to n steps from step k and
// returns how many it enqueued.  The chunk schedule depends on the call's arguments and the handle's
// configuration only — never on whether this handle is in the steady fused state: a chunk
// covers min(steps left, steps per launch) steps on every rank, and a handle that is not steady runs the
// chunk's first step alone and the rest as a second launch into the same chunk, so every rank issues the
// same all-gathers with the same sizes and the same step layout.
template <class StepFn>
void recordsLoop(mrts_env* env, int32_t n_steps, const int32_t* d_obs, uint32_t* d_recv, int64_t* offsets, void* stream,
                 StepFn step) {
    if (!exInited(env)) throw Fail{-EINVAL, "mrts_exchange_init first"};
    if (!env->recUnits) throw Fail{-EINVAL, "mrts_set_records first"};
    // a partially observable record holds the views' snapshot, which the step takes as part of its
    // observation write (an auto-reset's fresh snapshot too): without d_obs it would be empty
    if (env->partialObs && !d_obs) throw Fail{-EINVAL, "partially observable records need an observation buffer (d_obs)"};
    if (!d_recv || ((uintptr_t)d_recv & 15)) throw Fail{-EINVAL, "the receive buffer must be non-null and 16-byte aligned"};
    // (partially observable records carry hp as int8: the kernel flags a value outside the record's range)
    if (!env->obsImg && !env->partialObs) throw Fail{-ENOTSUP, "records: an observation value no longer fits a byte"};
    HIPCHK(hipSetDevice(env->device));
    hipStream_t s = pickStream(env, stream);
    const size_t per = (size_t)env->nGames * recWords(env->recUnits, env->partialObs);  // words per rank and step
    size_t base = 0;                                                   // words of d_recv filled so far
    bool any = false;
    const int32_t cap = env->multiStep ? (env->recSteps > 0 ? env->recSteps : MRTS_MAX_ITER) : 1;
    for (int32_t k = 0; k < n_steps;) {
        const int32_t n = std::min<int32_t>(n_steps - k, cap);  // the chunk's steps, the same on every rank
        for (int32_t j = 0; j < n;) {
            const RecPlan rp{d_recv + base, env->exRank, n, j};
            j += step(k + j, n - j, &rp);
        }
        HIPCHK(hipEventRecord(env->exReady[0], s));
        HIPCHK(hipStreamWaitEvent(env->exStream, env->exReady[0], 0));
        const size_t words = (size_t)n * per;
        exAllGather(env, d_recv + base + (size_t)env->exRank * words, d_recv + base, words * 4,
                    4 * (size_t)recWords(env->recUnits, env->partialObs), (size_t)env->nGames);  // (loopback: rotate games)
        if (offsets)
            for (int32_t j = 0; j < n; j++) {
                offsets[2 * (size_t)(k + j)] = (int64_t)(base + (size_t)j * per);
                offsets[2 * (size_t)(k + j) + 1] = (int64_t)words;
            }
        base += (size_t)env->exRanks * words;
        k += n;
        any = true;
    }
    if (any) {  // the caller's stream covers every collective of the call
        HIPCHK(hipEventRecord(env->exDone[0], env->exStream));
        HIPCHK(hipStreamWaitEvent(s, env->exDone[0], 0));
    }
}
}  // namespace
extern "C" {

int mrts_set_records(mrts_env* env, int32_t units_per_record, int32_t steps_per_launch) {
    return guarded(env, [&] {
        if (units_per_record == 0) {
            env->recUnits = 0;
            return 0;
        }
        if (units_per_record < 1 || units_per_record > 0xFFFF || steps_per_launch < 0)
            throw Fail{-EINVAL, "units per record 1..65535, steps per launch >= 0"};
        if (env->nSpGames != env->nGames || (env->HW & 3))
            throw Fail{-ENOTSUP, "records: self-play handles, maps whose cell count is a multiple of 4"};
        if (!env->partialObs && (env->HW > 256 || env->utt.ntypes > 7 || !env->obsImg))
            throw Fail{-ENOTSUP, "records (full observability): maps of <= 256 cells, <= 7 unit types, every observation "
                                 "value < 256"};
        if (env->partialObs && (env->HW > 65536 || env->utt.ntypes > 15 || env->hstatic.C != 8 ||
                                4 * (size_t)(2 * env->HW + 4 * env->H * ((env->W + 31) / 32) + recWords(units_per_record, true)) >
                                    64 * 1024))
            throw Fail{-ENOTSUP, "records (partial observability): <= 15 unit types, the receiver's render state and one "
                                 "record in 64 KB of LDS"};
        // the renders' overflow flag: allocated and zeroed here, never on a render path (a lazy
        // hipMalloc there would break a stream capture, and a null-stream memset is unordered with a
        // non-blocking render stream)
        if (!env->d_renderErr) {
            HIPCHK(hipSetDevice(env->device));
            HIPCHK(hipMalloc(&env->d_renderErr, 4));
            HIPCHK(hipMemset(env->d_renderErr, 0, 4));
            HIPCHK(hipDeviceSynchronize());
        }
        env->recUnits = units_per_record;
        env->recSteps = steps_per_launch;
        return 0;
    });
}

int mrts_rollout_fused_records_dev(mrts_env* env, int32_t* d_actions, const int32_t* d_players, int32_t* d_obs,
                                   double* d_reward, uint8_t* d_done, uint8_t* d_masks, int32_t mask_player, uint64_t seed,
                                   uint32_t first_next_step, int32_t n_steps, uint32_t* d_recv, int64_t* step_offsets,
                                   void* stream) {
    return guarded(env, [&] {
        RespScope rs(env, n_steps);
        RolloutEvents ev(env, stream);
        recordsLoop(env, n_steps, d_obs, d_recv, step_offsets, stream, [&](int32_t k, int32_t n, const RecPlan* rp) {
            return stepFused(env, d_actions, d_players, d_obs, d_reward, d_done, d_masks, mask_player, seed,
                             first_next_step + (uint32_t)k, n, stream, nullptr, nullptr, rp);
        });
        ev.done();
        return 0;
    });
}

int mrts_rollout_uniform_records_dev(mrts_env* env, int32_t* d_actions, const int32_t* d_players, int32_t* d_obs,
                                     double* d_reward, uint8_t* d_done, uint64_t seed, uint32_t first_step, int32_t n_steps,
                                     uint32_t* d_recv, int64_t* step_offsets, void* stream) {
    return guarded(env, [&] {
        RespScope rs(env, n_steps);
        RolloutEvents ev(env, stream);
        recordsLoop(env, n_steps, d_obs, d_recv, step_offsets, stream, [&](int32_t k, int32_t n, const RecPlan* rp) {
            return stepUniform(env, d_actions, d_players, d_obs, d_reward, d_done, nullptr, 0, seed, first_step + (uint32_t)k, n,
                               stream, nullptr, nullptr, rp);
        });
        ev.done();
        return 0;
    });
}

int mrts_render_records_onehot_dev(mrts_env* env, const uint32_t* d_rec, int64_t rec_words, int32_t n_ranks, int64_t rank_stride,
                                   const int32_t* d_sel, const int64_t* d_step_off, int32_t n_sel, uint8_t* d_out, void* stream) {
    return guarded(env, [&] {
        if (!d_rec || !d_out || (n_sel > 0 && !d_sel) || n_sel < 0 || rank_stride < 0 || rec_words < 0 || n_ranks < 1)
            throw Fail{-EINVAL, "bad argument"};
        if (!env->recUnits || !env->d_renderErr) throw Fail{-EINVAL, "mrts_set_records first"};
        if (env->partialObs) throw Fail{-ENOTSUP, "one-hot from records: full observability only"};
        if (((uintptr_t)d_out & 15) || ((uintptr_t)d_rec & 3)) throw Fail{-EINVAL, "misaligned buffer"};
        HIPCHK(hipSetDevice(env->device));
        HIPCHK(launchRenderRecordsOneHot(env->hstatic, env->d_static, d_rec, rec_words, n_ranks, env->recUnits, rank_stride, d_sel,
                                         d_step_off, n_sel, d_out, env->d_renderErr, pickStream(env, stream)));
        return 0;
    });
}

int mrts_render_status(mrts_env* env) {
    return guarded(env, [&] {
        if (!env->d_renderErr) return 0;
        HIPCHK(hipSetDevice(env->device));
        HIPCHK(hipDeviceSynchronize());
        int32_t v = 0;
        HIPCHK(hipMemcpy(&v, env->d_renderErr, 4, hipMemcpyDeviceToHost));
        if (v) HIPCHK(hipMemset(env->d_renderErr, 0, 4));
        return v ? 1 : 0;
    });
}

int32_t mrts_record_words(const mrts_env* env) {
    return guarded(env, [&] { return env->recUnits ? recWords(env->recUnits, env->partialObs) : 0; });
}

int mrts_render_records_dev(mrts_env* env, const uint32_t* d_rec, int64_t rec_words, int32_t n_ranks, int64_t rank_stride,
                            void* d_out, int32_t out_bytes, void* stream) {
    return guarded(env, [&] {
        if (!d_rec || !d_out || n_ranks < 1 || rank_stride < 0 || rec_words < 0) throw Fail{-EINVAL, "bad argument"};
        if (!env->recUnits || !env->d_renderErr) throw Fail{-EINVAL, "mrts_set_records first"};
        if (out_bytes != 1 && out_bytes != 4) throw Fail{-EINVAL, "out_bytes: 1 (uint8) or 4 (int32)"};
        if (((uintptr_t)d_out & (out_bytes == 4 ? 15 : 3)) || ((uintptr_t)d_rec & 3)) throw Fail{-EINVAL, "misaligned buffer"};
        // every rank's records inside the buffer (the kernel reads n_games records per rank)
        const int64_t span = (int64_t)(n_ranks - 1) * rank_stride + (int64_t)env->nGames * recWords(env->recUnits, env->partialObs);
        if (span > rec_words) throw Fail{-EINVAL, "the ranks' records reach past the receive buffer (rec_words)"};
        HIPCHK(hipSetDevice(env->device));
        HIPCHK(launchRenderRecords(env->hstatic, env->d_static, d_rec, env->recUnits, n_ranks, rank_stride, d_out, out_bytes,
                                   env->d_renderErr, pickStream(env, stream)));
        return 0;
    });
}

int mrts_capture_begin(mrts_env* env, void* stream) {
    return guarded(env, [&] {
        if (!stream) throw Fail{-EINVAL, "capture needs a handle and a non-default stream"};
        HIPCHK(hipSetDevice(env->device));
        HIPCHK(hipStreamBeginCapture((hipStream_t)stream, hipStreamCaptureModeThreadLocal));
        return 0;
    });
}

int mrts_capture_end(mrts_env* env, void* stream) {
    return guarded(env, [&] {
        if (!stream) throw Fail{-EINVAL, "capture needs a handle and a non-default stream"};
        hipGraph_t g = nullptr;
        HIPCHK(hipStreamEndCapture((hipStream_t)stream, &g));
        if (env->capExec) (void)hipGraphExecDestroy(env->capExec);
        if (env->capGraph) (void)hipGraphDestroy(env->capGraph);
        env->capExec = nullptr;
        env->capGraph = g;
        HIPCHK(hipGraphInstantiate(&env->capExec, g, nullptr, nullptr, 0));
        return 0;
    });
}

int mrts_replay(mrts_env* env, void* stream) {
    return guarded(env, [&] {
        if (!env->capExec) throw Fail{-EINVAL, "nothing captured"};
        HIPCHK(hipSetDevice(env->device));
        HIPCHK(hipGraphLaunch(env->capExec, pickStream(env, stream)));
        return 0;
    });
}

int mrts_rccl_unique_id(const char* rccl_path, void* out) {
    return guardedCall([&] {
        if (!out) throw Fail{-EINVAL, "null argument"};
        loadRccl(rccl_path);
        ncclUniqueId id;
        ncclChk(g_rccl.getUniqueId(&id), "ncclGetUniqueId");
        std::memcpy(out, &id, sizeof(id));
        return 0;
    });
}

namespace {
// the exchange's own stream and per send buffer its step-ready / collective-done events
void exchangeStreams(mrts_env* env) {
    HIPCHK(hipStreamCreateWithFlags(&env->exStream, hipStreamNonBlocking));
    for (int b = 0; b < 2; b++) {
        HIPCHK(hipEventCreateWithFlags(&env->exReady[b], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&env->exDone[b], hipEventDisableTiming));
    }
}
}  // namespace

int mrts_exchange_init(mrts_env* env, const char* rccl_path, int32_t nranks, int32_t rank, const void* unique_id) {
    return guarded(env, [&] {
        if (!unique_id || nranks < 1 || rank < 0 || rank >= nranks) throw Fail{-EINVAL, "bad exchange arguments"};
        if (exInited(env)) throw Fail{-EINVAL, "the exchange is already initialised"};
        loadRccl(rccl_path);
        HIPCHK(hipSetDevice(env->device));
        ncclUniqueId id;
        std::memcpy(&id, unique_id, sizeof(id));
        ncclChk(g_rccl.commInitRank(&env->exComm, nranks, id, rank), "ncclCommInitRank");
        env->exRanks = nranks;
        env->exRank = rank;
        exchangeStreams(env);
        return 0;
    });
}

int mrts_exchange_init_loopback(mrts_env* env, int32_t nranks, int32_t rank) {
    return guarded(env, [&] {
        if (nranks < 1 || rank < 0 || rank >= nranks) throw Fail{-EINVAL, "bad exchange arguments"};
        if (exInited(env)) throw Fail{-EINVAL, "the exchange is already initialised"};
        HIPCHK(hipSetDevice(env->device));
        exchangeStreams(env);
        env->exRanks = nranks;
        env->exRank = rank;
        env->exLoop = true;
        return 0;
    });
}

int mrts_rollout_fused_exchange_dev(mrts_env* env, int32_t* d_actions, const int32_t* d_players, int32_t* d_obs,
                                    double* d_reward, uint8_t* d_done, uint8_t* d_masks, int32_t mask_player, uint64_t seed,
                                    uint32_t first_next_step, int32_t n_steps, int16_t* d_send0, int16_t* d_send1,
                                    int16_t* d_recv, void* stream) {
    return guarded(env, [&] {
        RespScope rs(env, n_steps);
        RolloutEvents ev(env, stream);
        exchangeLoop(env, n_steps, d_obs, d_send0, d_send1, d_recv, stream, [&](int32_t k) {
            stepFused(env, d_actions, d_players, d_obs, d_reward, d_done, d_masks, mask_player, seed,
                      first_next_step + (uint32_t)k, 1, stream);
        });
        ev.done();
        return 0;
    });
}

int mrts_rollout_uniform_exchange_dev(mrts_env* env, int32_t* d_actions, const int32_t* d_players, int32_t* d_obs,
                                      double* d_reward, uint8_t* d_done, uint64_t seed, uint32_t first_step, int32_t n_steps,
                                      int16_t* d_send0, int16_t* d_send1, int16_t* d_recv, void* stream) {
    return guarded(env, [&] {
        RespScope rs(env, n_steps);
        RolloutEvents ev(env, stream);
        exchangeLoop(env, n_steps, d_obs, d_send0, d_send1, d_recv, stream, [&](int32_t k) {
            stepUniform(env, d_actions, d_players, d_obs, d_reward, d_done, nullptr, 0, seed, first_step + (uint32_t)k, 1,
                        stream);
        });
        ev.done();
        return 0;
    });
}

int mrts_policy_invalidate(mrts_env* env) {
    return guarded(env, [&] {
        env->polValid = false;
        env->fusedActions = nullptr;
        return 0;
    });
}

int mrts_set_obs_delta(mrts_env* env, int32_t on) {
    return guarded(env, [&] {
        env->obsDelta = on ? 1 : 0;
        env->lastObsPtr = nullptr;
        return 0;
    });
}

int mrts_set_exchange_bytes(mrts_env* env, int32_t bytes_per_value) {
    return guarded(env, [&] {
        if (bytes_per_value == 2) {
            env->exBytes = 2;
            return 0;
        }
        if (bytes_per_value != 1) throw Fail{-EINVAL, "bytes per value: 1 or 2"};
        // the uint8 transport is written by the 16x16 byte-image render and the one-cell-per-lane render of
        // maps of <= 64 cells: full observability whose every value fits a byte (checked at create over the
        // maps and the unit-type table)
        if (env->partialObs || !(env->HW == 256 || env->HW <= 64) || !env->obsImg)
            throw Fail{-ENOTSUP, "uint8 exchange: full observability on 16x16 or <= 64-cell maps, every value < 256"};
        env->exBytes = 1;
        return 0;
    });
}

int mrts_set_obs16(mrts_env* env, int16_t* d_obs16) {
    return guarded(env, [&] {
        if (d_obs16 && env->partialObs) throw Fail{-EINVAL, "the int16 observation copy is for full observability"};
        if ((uintptr_t)d_obs16 & 7) throw Fail{-EINVAL, "misaligned buffer (8 bytes)"};
        env->obs16 = d_obs16;
        return 0;
    });
}

int mrts_obs_invalidate(mrts_env* env) {
    return guarded(env, [&] {
        env->lastObsPtr = nullptr;
        return 0;
    });
}

int mrts_set_source_output(mrts_env* env, uint32_t* d_source) {
    return guarded(env, [&] {
        env->d_source = d_source;
        return 0;
    });
}

int mrts_policy_dev(mrts_env* env, const uint8_t* d_masks, const uint32_t* d_source, uint64_t seed, uint32_t step,
                    int32_t* d_actions, void* stream) {
    return guarded(env, [&] {
        HIPCHK(hipSetDevice(env->device));
        PolicyParams Q;
        Q.HW = env->HW;
        Q.K = env->K;
        Q.ntypes = env->utt.ntypes;
        Q.n_slots = env->nSlots;
        Q.slot_id_base = env->slotIdBase;
        Q.step = step;
        Q.seed = seed;
        Q.masks = d_masks;
        Q.source = d_source;
        Q.actions = d_actions;
        Q.prev = nullptr;
        Q.prev_out = nullptr;
        Q.delta = 0;
        const size_t pw = (size_t)env->nSlots * maskWords(env->HW);
        if (d_source && env->maskDelta) {  // double-buffered candidate sets: read one, write the other
            if (!env->d_polPrev) HIPCHK(hipMalloc(&env->d_polPrev, 2 * pw * 4));
            Q.prev = env->d_polPrev + pw * env->polParity;
            Q.prev_out = env->d_polPrev + pw * (1 - env->polParity);
            Q.delta = (env->polValid && d_actions == env->lastPolicyActions) ? 1 : 0;
        }
        bool prevWritten = false;
        if (d_actions == env->fusedActions) env->fusedActions = nullptr;
        HIPCHK(launchPolicy(Q, pickStream(env, stream), &prevWritten));
        env->polValid = prevWritten;
        if (prevWritten) env->polParity ^= 1;
        env->lastPolicyActions = d_actions;
        return 0;
    });
}

namespace {
static_assert(HEAD_LT_F32 == MRTS_LOGITS_F32 && HEAD_LT_BF16 == MRTS_LOGITS_BF16 && HEAD_LT_F16 == MRTS_LOGITS_F16,
              "the kernels' element types are include/mrts.h's");
// the logits' element type of a typed call: its alignment mask (a 16-bit buffer needs 2-byte alignment only)
uintptr_t headLogitAlign(int32_t ltype) {
    if (ltype != HEAD_LT_F32 && ltype != HEAD_LT_BF16 && ltype != HEAD_LT_F16)
        throw Fail{-EINVAL, "logits_type: MRTS_LOGITS_F32, MRTS_LOGITS_BF16 or MRTS_LOGITS_F16"};
    return (uintptr_t)headLogitBytes(ltype) - 1;
}
// the policy head's shared argument checks; n_rows rows of the handle's H*W cells, logits of element type ltype
HeadParams headParams(mrts_env* env, int32_t n_rows, int32_t ltype, const void* d_logits, const uint8_t* d_masks,
                      const int32_t* d_actions) {
    const uintptr_t lmask = headLogitAlign(ltype);
    if (env->botOnly || env->forwardModel)
        throw Fail{-ENOTSUP, "the policy head needs a handle that writes masks (not a bot-only or forward-model handle)"};
    if (!d_logits || !d_masks || !d_actions) throw Fail{-EINVAL, "null argument"};
    if (n_rows < 0 || (int64_t)n_rows * env->HW >= ((int64_t)1 << 31)) throw Fail{-EINVAL, "n_rows: 0 <= n_rows * H*W < 2^31"};
    if (((uintptr_t)d_logits & lmask) || ((uintptr_t)d_actions & 3)) throw Fail{-EINVAL, "misaligned buffer"};
    const int nt = env->utt.ntypes, natt = env->K - 23 - nt;
    if (env->K - 1 > HEAD_MAX_LOGITS || nt > 16 || natt < 0 || natt > 64)
        throw Fail{-ENOTSUP, "the policy head: at most 16 unit types, 64 attack-window cells and 80 logits per cell"};
    HeadParams Q;
    std::memset(&Q, 0, sizeof(Q));
    Q.HW = env->HW;
    Q.K = env->K;
    Q.ntypes = nt;
    Q.n_rows = n_rows;
    Q.slot_id_base = env->slotIdBase;
    Q.logits = d_logits;
    Q.ltype = ltype;
    Q.masks = d_masks;
    Q.actions = const_cast<int32_t*>(d_actions);
    return Q;
}

// the three dense calls, for the float32 entry points (ltype MRTS_LOGITS_F32) and the typed ones alike
int headSample(mrts_env* env, int32_t ltype, const void* d_logits, const uint8_t* d_masks, const uint32_t* d_source,
               uint64_t seed, uint32_t step, int32_t* d_actions, float* d_logprob, float* d_entropy, void* stream) {
    return guarded(env, [&] {
        HeadParams Q = headParams(env, env->nSlots, ltype, d_logits, d_masks, d_actions);
        if (((uintptr_t)d_source & 3) || ((uintptr_t)d_logprob & 3) || ((uintptr_t)d_entropy & 3)) throw Fail{-EINVAL, "misaligned buffer"};
        HIPCHK(hipSetDevice(env->device));
        Q.source = d_source;
        Q.seed = seed;
        Q.step = step;
        Q.logprob = d_logprob;
        Q.entropy = d_entropy;
        // the rows are no longer what the masked-uniform policy or a fused step wrote (mrts_policy_invalidate)
        env->polValid = false;
        env->fusedActions = nullptr;
        HIPCHK(launchHead(HEAD_SAMPLE, Q, pickStream(env, stream)));
        return 0;
    });
}

int headScore(mrts_env* env, int32_t n_rows, int32_t ltype, const void* d_logits, const uint8_t* d_masks,
              const int32_t* d_actions, float* d_logprob, float* d_entropy, void* stream) {
    return guarded(env, [&] {
        HeadParams Q = headParams(env, n_rows, ltype, d_logits, d_masks, d_actions);
        if (((uintptr_t)d_logprob & 3) || ((uintptr_t)d_entropy & 3)) throw Fail{-EINVAL, "misaligned buffer"};
        HIPCHK(hipSetDevice(env->device));
        Q.logprob = d_logprob;
        Q.entropy = d_entropy;
        HIPCHK(launchHead(HEAD_SCORE, Q, pickStream(env, stream)));
        return 0;
    });
}

int headGrad(mrts_env* env, int32_t n_rows, int32_t ltype, const void* d_logits, const uint8_t* d_masks,
             const int32_t* d_actions, const float* d_g_logprob, const float* d_g_entropy, void* d_grad_logits, void* stream) {
    return guarded(env, [&] {
        HeadParams Q = headParams(env, n_rows, ltype, d_logits, d_masks, d_actions);
        if (!d_grad_logits) throw Fail{-EINVAL, "null argument"};
        if (((uintptr_t)d_g_logprob & 3) || ((uintptr_t)d_g_entropy & 3) || ((uintptr_t)d_grad_logits & headLogitAlign(ltype)))
            throw Fail{-EINVAL, "misaligned buffer"};
        HIPCHK(hipSetDevice(env->device));
        Q.g_logprob = d_g_logprob;
        Q.g_entropy = d_g_entropy;
        Q.grad = d_grad_logits;
        HIPCHK(launchHead(HEAD_GRAD, Q, pickStream(env, stream)));
        return 0;
    });
}
}  // namespace

int mrts_policy_head_sample_dev(mrts_env* env, const float* d_logits, const uint8_t* d_masks, const uint32_t* d_source,
                                uint64_t seed, uint32_t step, int32_t* d_actions, float* d_logprob, float* d_entropy,
                                void* stream) {
    return headSample(env, MRTS_LOGITS_F32, d_logits, d_masks, d_source, seed, step, d_actions, d_logprob, d_entropy, stream);
}
int mrts_policy_head_sample_typed_dev(mrts_env* env, int32_t logits_type, const void* d_logits, const uint8_t* d_masks,
                                      const uint32_t* d_source, uint64_t seed, uint32_t step, int32_t* d_actions,
                                      float* d_logprob, float* d_entropy, void* stream) {
    return headSample(env, logits_type, d_logits, d_masks, d_source, seed, step, d_actions, d_logprob, d_entropy, stream);
}

int mrts_policy_head_score_dev(mrts_env* env, int32_t n_rows, const float* d_logits, const uint8_t* d_masks,
                               const int32_t* d_actions, float* d_logprob, float* d_entropy, void* stream) {
    return headScore(env, n_rows, MRTS_LOGITS_F32, d_logits, d_masks, d_actions, d_logprob, d_entropy, stream);
}
int mrts_policy_head_score_typed_dev(mrts_env* env, int32_t n_rows, int32_t logits_type, const void* d_logits,
                                     const uint8_t* d_masks, const int32_t* d_actions, float* d_logprob, float* d_entropy,
                                     void* stream) {
    return headScore(env, n_rows, logits_type, d_logits, d_masks, d_actions, d_logprob, d_entropy, stream);
}

int mrts_policy_head_grad_dev(mrts_env* env, int32_t n_rows, const float* d_logits, const uint8_t* d_masks,
                              const int32_t* d_actions, const float* d_g_logprob, const float* d_g_entropy,
                              float* d_grad_logits, void* stream) {
    return headGrad(env, n_rows, MRTS_LOGITS_F32, d_logits, d_masks, d_actions, d_g_logprob, d_g_entropy, d_grad_logits, stream);
}
int mrts_policy_head_grad_typed_dev(mrts_env* env, int32_t n_rows, int32_t logits_type, const void* d_logits,
                                    const uint8_t* d_masks, const int32_t* d_actions, const float* d_g_logprob,
                                    const float* d_g_entropy, void* d_grad_logits, void* stream) {
    return headGrad(env, n_rows, logits_type, d_logits, d_masks, d_actions, d_g_logprob, d_g_entropy, d_grad_logits, stream);
}

namespace {
// the packed rows' shared argument checks: the handle as headParams wants it, n_rows rows of H*W cells, 1 <= cap <= H*W
HeadPackedParams headPackedParams(mrts_env* env, int32_t n_rows, int32_t cap) {
    if (env->botOnly || env->forwardModel)
        throw Fail{-ENOTSUP, "the policy head needs a handle that writes masks (not a bot-only or forward-model handle)"};
    if (n_rows < 0 || (int64_t)n_rows * env->HW >= ((int64_t)1 << 31)) throw Fail{-EINVAL, "n_rows: 0 <= n_rows * H*W < 2^31"};
    if (cap < 1 || cap > env->HW) throw Fail{-EINVAL, "cap: 1 <= cap <= H*W"};
    const int nt = env->utt.ntypes, natt = env->K - 23 - nt;
    if (env->K - 1 > HEAD_MAX_LOGITS || nt > 16 || natt < 0 || natt > 64)
        throw Fail{-ENOTSUP, "the policy head: at most 16 unit types, 64 attack-window cells and 80 logits per cell"};
    HeadPackedParams P;
    std::memset(&P, 0, sizeof(P));
    P.H.HW = env->HW;
    P.H.K = env->K;
    P.H.ntypes = nt;
    P.H.n_rows = n_rows;
    P.H.slot_id_base = env->slotIdBase;
    P.cap = cap;
    P.words = headPackedWords(cap);
    return P;
}
// packed rows as a score / gradient / unpack call reads them: without an index row r reads packed row r
void headPackedSource(HeadPackedParams& P, const uint32_t* d_packed, int32_t n_packed, const int32_t* d_index) {
    if (!d_packed) throw Fail{-EINVAL, "null argument"};
    if (n_packed < 1 || (!d_index && n_packed < P.H.n_rows)) throw Fail{-EINVAL, "n_packed: at least 1, and n_rows without an index"};
    if (((uintptr_t)d_packed & 3) || ((uintptr_t)d_index & 3)) throw Fail{-EINVAL, "misaligned buffer"};
    P.packed = d_packed;
    P.n_packed = n_packed;
    P.index = d_index;
}
}  // namespace

int32_t mrts_policy_head_packed_words(const mrts_env* env, int32_t cap) {
    return guarded(env, [&] {
        if (env->botOnly || env->forwardModel) throw Fail{-ENOTSUP, "the policy head needs a handle that writes masks"};
        if (cap < 1 || cap > env->HW) throw Fail{-EINVAL, "cap: 1 <= cap <= H*W"};
        return headPackedWords(cap);
    });
}

int mrts_policy_head_pack_dev(mrts_env* env, int32_t n_rows, const uint8_t* d_masks, const uint32_t* d_source,
                              const int32_t* d_actions, int32_t cap, uint32_t* d_packed, void* stream) {
    return guarded(env, [&] {
        HeadPackedParams P = headPackedParams(env, n_rows, cap);
        if (!d_masks || !d_actions || !d_packed) throw Fail{-EINVAL, "null argument"};
        if (((uintptr_t)d_source & 3) || ((uintptr_t)d_actions & 3) || ((uintptr_t)d_packed & 3)) throw Fail{-EINVAL, "misaligned buffer"};
        HIPCHK(hipSetDevice(env->device));
        if (!env->d_packOverflow) {
            HIPCHK(hipMalloc(&env->d_packOverflow, 8));
            HIPCHK(hipMemset(env->d_packOverflow, 0, 8));
        }
        P.H.masks = d_masks;
        P.H.source = d_source;
        P.H.actions = const_cast<int32_t*>(d_actions);
        P.packed_out = d_packed;
        P.overflow = env->d_packOverflow;
        HIPCHK(launchHeadPacked(HEAD_PACK, P, pickStream(env, stream)));
        return 0;
    });
}

int mrts_policy_head_pack_status(mrts_env* env, int64_t* overflow_rows) {
    return guarded(env, [&] {
        if (!overflow_rows) throw Fail{-EINVAL, "null argument"};
        *overflow_rows = 0;
        if (!env->d_packOverflow) return 0;
        HIPCHK(hipSetDevice(env->device));
        HIPCHK(hipDeviceSynchronize());
        unsigned long long v = 0;
        HIPCHK(hipMemcpy(&v, env->d_packOverflow, 8, hipMemcpyDeviceToHost));
        if (v) HIPCHK(hipMemset(env->d_packOverflow, 0, 8));
        *overflow_rows = (int64_t)v;
        return 0;
    });
}

int mrts_policy_head_unpack_dev(mrts_env* env, int32_t n_rows, const uint32_t* d_packed, int32_t n_packed, int32_t cap,
                                const int32_t* d_index, uint8_t* d_masks_out, int32_t* d_actions_out, void* stream) {
    return guarded(env, [&] {
        HeadPackedParams P = headPackedParams(env, n_rows, cap);
        headPackedSource(P, d_packed, n_packed, d_index);
        if (!d_masks_out || !d_actions_out) throw Fail{-EINVAL, "null argument"};
        if ((uintptr_t)d_actions_out & 3) throw Fail{-EINVAL, "misaligned buffer"};
        HIPCHK(hipSetDevice(env->device));
        P.masks_out = d_masks_out;
        P.actions_out = d_actions_out;
        HIPCHK(launchHeadPacked(HEAD_UNPACK, P, pickStream(env, stream)));
        return 0;
    });
}

namespace {
// the two calls that score packed rows, for the float32 entry points and the typed ones alike
int headScorePacked(mrts_env* env, int32_t n_rows, int32_t ltype, const void* d_logits, const uint32_t* d_packed,
                    int32_t n_packed, int32_t cap, const int32_t* d_index, float* d_logprob, float* d_entropy, void* stream) {
    return guarded(env, [&] {
        const uintptr_t lmask = headLogitAlign(ltype);
        HeadPackedParams P = headPackedParams(env, n_rows, cap);
        headPackedSource(P, d_packed, n_packed, d_index);
        if (!d_logits) throw Fail{-EINVAL, "null argument"};
        if (((uintptr_t)d_logits & lmask) || ((uintptr_t)d_logprob & 3) || ((uintptr_t)d_entropy & 3)) throw Fail{-EINVAL, "misaligned buffer"};
        HIPCHK(hipSetDevice(env->device));
        P.H.logits = d_logits;
        P.H.ltype = ltype;
        P.H.logprob = d_logprob;
        P.H.entropy = d_entropy;
        HIPCHK(launchHeadPacked(HEAD_SCORE, P, pickStream(env, stream)));
        return 0;
    });
}

int headGradPacked(mrts_env* env, int32_t n_rows, int32_t ltype, const void* d_logits, const uint32_t* d_packed,
                   int32_t n_packed, int32_t cap, const int32_t* d_index, const float* d_g_logprob, const float* d_g_entropy,
                   void* d_grad_logits, void* stream) {
    return guarded(env, [&] {
        const uintptr_t lmask = headLogitAlign(ltype);
        HeadPackedParams P = headPackedParams(env, n_rows, cap);
        headPackedSource(P, d_packed, n_packed, d_index);
        if (!d_logits || !d_grad_logits) throw Fail{-EINVAL, "null argument"};
        if (((uintptr_t)d_logits & lmask) || ((uintptr_t)d_g_logprob & 3) || ((uintptr_t)d_g_entropy & 3) || ((uintptr_t)d_grad_logits & lmask))
            throw Fail{-EINVAL, "misaligned buffer"};
        HIPCHK(hipSetDevice(env->device));
        P.H.logits = d_logits;
        P.H.ltype = ltype;
        P.H.g_logprob = d_g_logprob;
        P.H.g_entropy = d_g_entropy;
        P.H.grad = d_grad_logits;
        HIPCHK(launchHeadPacked(HEAD_GRAD, P, pickStream(env, stream)));
        return 0;
    });
}
}  // namespace

int mrts_policy_head_score_packed_dev(mrts_env* env, int32_t n_rows, const float* d_logits, const uint32_t* d_packed,
                                      int32_t n_packed, int32_t cap, const int32_t* d_index, float* d_logprob,
                                      float* d_entropy, void* stream) {
    return headScorePacked(env, n_rows, MRTS_LOGITS_F32, d_logits, d_packed, n_packed, cap, d_index, d_logprob, d_entropy, stream);
}
int mrts_policy_head_score_packed_typed_dev(mrts_env* env, int32_t n_rows, int32_t logits_type, const void* d_logits,
                                            const uint32_t* d_packed, int32_t n_packed, int32_t cap, const int32_t* d_index,
                                            float* d_logprob, float* d_entropy, void* stream) {
    return headScorePacked(env, n_rows, logits_type, d_logits, d_packed, n_packed, cap, d_index, d_logprob, d_entropy, stream);
}

int mrts_policy_head_grad_packed_dev(mrts_env* env, int32_t n_rows, const float* d_logits, const uint32_t* d_packed,
                                     int32_t n_packed, int32_t cap, const int32_t* d_index, const float* d_g_logprob,
                                     const float* d_g_entropy, float* d_grad_logits, void* stream) {
    return headGradPacked(env, n_rows, MRTS_LOGITS_F32, d_logits, d_packed, n_packed, cap, d_index, d_g_logprob, d_g_entropy,
                          d_grad_logits, stream);
}
int mrts_policy_head_grad_packed_typed_dev(mrts_env* env, int32_t n_rows, int32_t logits_type, const void* d_logits,
                                           const uint32_t* d_packed, int32_t n_packed, int32_t cap, const int32_t* d_index,
                                           const float* d_g_logprob, const float* d_g_entropy, void* d_grad_logits,
                                           void* stream) {
    return headGradPacked(env, n_rows, logits_type, d_logits, d_packed, n_packed, cap, d_index, d_g_logprob, d_g_entropy,
                          d_grad_logits, stream);
}

// ---- packed observation rows (include/mrts.h; the argument checks are mrts_hostdata.cpp's)
namespace {
// the counters of mrts_obs_packed_status, allocated at the first call outside a capture (an allocation and a memset
// cannot be captured): a first call inside one is refused
void obsPackCounters(mrts_env* env, hipStream_t s) {
    if (env->d_obsPackCnt) return;
    hipStreamCaptureStatus cst = hipStreamCaptureStatusNone;
    HIPCHK(hipStreamIsCapturing(s, &cst));
    if (cst != hipStreamCaptureStatusNone)
        throw Fail{-EINVAL, "packed observation rows: make the first call (mrts_obs_packed_status will do) outside a capture"};
    HIPCHK(hipMalloc(&env->d_obsPackCnt, 16));
    HIPCHK(hipMemset(env->d_obsPackCnt, 0, 16));
}
}  // namespace

int32_t mrts_obs_packed_words(const mrts_env* env, int32_t cap) {
    return guarded(env, [&] { return obsPackShape(*env, 0, cap).words; });
}

int mrts_obs_pack_dev(mrts_env* env, int32_t n_rows, const int32_t* d_obs, int32_t cap, uint32_t* d_out, void* stream) {
    return guarded(env, [&] {
        ObsPackParams P = obsPackShape(*env, n_rows, cap);
        obsPackBuffers(P, d_obs, d_out);
        HIPCHK(hipSetDevice(env->device));
        obsPackCounters(env, pickStream(env, stream));
        P.counters = env->d_obsPackCnt;
        HIPCHK(launchObsPacked(OBS_PACK, P, env->utt.ntypes, pickStream(env, stream)));
        return 0;
    });
}

int mrts_obs_unpack_dev(mrts_env* env, int32_t n_rows, const uint32_t* d_packed, int32_t n_packed, int32_t cap,
                        const int32_t* d_index, int32_t* d_obs, void* stream) {
    return guarded(env, [&] {
        ObsPackParams P = obsPackShape(*env, n_rows, cap);
        obsPackedSource(P, d_packed, n_packed, d_index, d_obs, 4);
        HIPCHK(hipSetDevice(env->device));
        obsPackCounters(env, pickStream(env, stream));
        P.counters = env->d_obsPackCnt;
        P.obs_out = d_obs;
        HIPCHK(launchObsPacked(OBS_UNPACK, P, env->utt.ntypes, pickStream(env, stream)));
        return 0;
    });
}

int mrts_obs_onehot_packed_dev(mrts_env* env, int32_t n_rows, const uint32_t* d_packed, int32_t n_packed, int32_t cap,
                               const int32_t* d_index, uint8_t* d_out, void* stream) {
    return guarded(env, [&] {
        ObsPackParams P = obsPackShape(*env, n_rows, cap);
        obsPackedSource(P, d_packed, n_packed, d_index, d_out, 16);
        HIPCHK(hipSetDevice(env->device));
        obsPackCounters(env, pickStream(env, stream));
        P.counters = env->d_obsPackCnt;
        P.onehot_out = d_out;
        HIPCHK(launchObsPacked(OBS_ONEHOT, P, env->utt.ntypes, pickStream(env, stream)));
        return 0;
    });
}

int mrts_obs_packed_status(mrts_env* env, int64_t* lossy_rows, int64_t* bad_reads) {
    return guarded(env, [&] {
        if (!lossy_rows || !bad_reads) throw Fail{-EINVAL, "null argument"};
        HIPCHK(hipSetDevice(env->device));
        obsPackCounters(env, nullptr);
        HIPCHK(hipDeviceSynchronize());
        unsigned long long v[2] = {0, 0};
        HIPCHK(hipMemcpy(v, env->d_obsPackCnt, 16, hipMemcpyDeviceToHost));
        if (v[0] | v[1]) HIPCHK(hipMemset(env->d_obsPackCnt, 0, 16));
        *lossy_rows = (int64_t)v[0];
        *bad_reads = (int64_t)v[1];
        return 0;
    });
}

static void fillResponses(mrts_env* env, mrts_responses* out) {
    const size_t S = (size_t)env->nSlots;
    HIPCHK(hipMemcpyAsync(env->h_obs, env->d_obs, S * env->C * env->HW * 4, hipMemcpyDeviceToHost, env->stream));
    const size_t R = env->rewardKinds.size();
    HIPCHK(hipMemcpyAsync(env->h_reward, env->d_reward, S * R * 8, hipMemcpyDeviceToHost, env->stream));
    HIPCHK(hipMemcpyAsync(env->h_done, env->d_done, S * R, hipMemcpyDeviceToHost, env->stream));
    HIPCHK(hipStreamSynchronize(env->stream));
    if (out) {
        out->obs = env->h_obs;
        out->reward = env->h_reward;
        out->done = env->h_done;
    }
}

// the host-pointer calls' players: the caller's, or zeros
static void stagePlayers(mrts_env* env, const int32_t* players) {
    const size_t S = (size_t)env->nSlots;
    if (players) HIPCHK(hipMemcpyAsync(env->d_players, players, S * 4, hipMemcpyHostToDevice, env->stream));
    else HIPCHK(hipMemsetAsync(env->d_players, 0, S * 4, env->stream));
}

int mrts_reset(mrts_env* env, const int32_t* players, mrts_responses* out) {
    return guarded(env, [&] {
        HIPCHK(hipSetDevice(env->device));
        stagePlayers(env, players);
        int r = mrts_reset_dev(env, env->d_players, env->d_obs, env->d_reward, env->d_done, nullptr, 0, env->stream);
        if (r) return r;
        fillResponses(env, out);
        return 0;
    });
}

int mrts_step(mrts_env* env, const int32_t* actions, const int32_t* players, mrts_responses* out) {
    return guarded(env, [&] {
        if (!actions) throw Fail{-EINVAL, "actions is null"};
        HIPCHK(hipSetDevice(env->device));
        const size_t S = (size_t)env->nSlots;
        HIPCHK(hipMemcpyAsync(env->d_actions, actions, S * env->HW * 7 * 4, hipMemcpyHostToDevice, env->stream));
        stagePlayers(env, players);
        int r = mrts_step_dev(env, env->d_actions, env->d_players, env->d_obs, env->d_reward, env->d_done, nullptr, 0, env->stream);
        if (r) return r;
        fillResponses(env, out);
        checkFlagsAfter(env);
        return 0;
    });
}

int mrts_step_rows(mrts_env* env, const int32_t* rows, int32_t n_rows, const int32_t* players, mrts_responses* out) {
    return guarded(env, [&] {
        if (!rows && n_rows > 0) throw Fail{-EINVAL, "rows is null"};
        if (n_rows < 0) throw Fail{-EINVAL, "bad n_rows"};
        HIPCHK(hipSetDevice(env->device));
        const size_t S = (size_t)env->nSlots, n = S * (size_t)n_rows * 8;
        if (n > env->rowsStageInts) {
            HIPCHK(hipStreamSynchronize(env->stream));
            (void)hipFree(env->d_rowsStage);
            env->d_rowsStage = nullptr;
            HIPCHK(hipMalloc(&env->d_rowsStage, n * 4));
            env->rowsStageInts = n;
        }
        if (n) HIPCHK(hipMemcpyAsync(env->d_rowsStage, rows, n * 4, hipMemcpyHostToDevice, env->stream));
        stagePlayers(env, players);
        int r = mrts_step_rows_dev(env, env->d_rowsStage, n_rows, env->d_players, env->d_obs, env->d_reward, env->d_done,
                                   nullptr, 0, env->stream);
        if (r) return r;
        fillResponses(env, out);
        checkFlagsAfter(env);
        return 0;
    });
}

int mrts_get_masks_i32(mrts_env* env, int32_t player, int32_t* out) {
    return guarded(env, [&] {
        if (!out) throw Fail{-EINVAL, "out is null"};
        const size_t n = (size_t)env->nSlots * env->HW * env->K;
        if (!env->d_masks32) HIPCHK(hipMalloc(&env->d_masks32, n * 4));
        int r = mrts_get_masks_i32_dev(env, player, env->d_masks32, env->stream);
        if (r) return r;
        HIPCHK(hipMemcpyAsync(out, env->d_masks32, n * 4, hipMemcpyDeviceToHost, env->stream));
        HIPCHK(hipStreamSynchronize(env->stream));
        return 0;
    });
}

int mrts_get_masks(mrts_env* env, int32_t player, uint8_t* out) {
    return guarded(env, [&] {
        if (!out) throw Fail{-EINVAL, "out is null"};
        int r = mrts_get_masks_dev(env, player, env->d_masks, env->stream);
        if (r) return r;
        HIPCHK(hipMemcpyAsync(out, env->d_masks, (size_t)env->nSlots * env->HW * env->K, hipMemcpyDeviceToHost, env->stream));
        HIPCHK(hipStreamSynchronize(env->stream));
        return 0;
    });
}

// getMasks into a library-owned pinned buffer (valid until the next call on the handle, like the Java
// client's reused mask array, JNIGridnetClient.java:211-215): the D2H copy runs at pinned-memory rate
// instead of staging through a pageable caller buffer
int mrts_get_masks_host(mrts_env* env, int32_t player, const uint8_t** out) {
    return guarded(env, [&] {
        if (!out) throw Fail{-EINVAL, "out is null"};
        const size_t n = (size_t)env->nSlots * env->HW * env->K;
        if (!env->h_masks) HIPCHK(hipHostMalloc(&env->h_masks, n, hipHostMallocDefault));
        int r = mrts_get_masks(env, player, env->h_masks);
        if (r) return r;
        *out = env->h_masks;
        return 0;
    });
}

int mrts_get_masks_i32_host(mrts_env* env, int32_t player, const int32_t** out) {
    return guarded(env, [&] {
        if (!out) throw Fail{-EINVAL, "out is null"};
        const size_t n = (size_t)env->nSlots * env->HW * env->K;
        if (!env->h_masks32) HIPCHK(hipHostMalloc(&env->h_masks32, n * 4, hipHostMallocDefault));
        int r = mrts_get_masks_i32(env, player, env->h_masks32);
        if (r) return r;
        *out = env->h_masks32;
        return 0;
    });
}

int mrts_get_state(mrts_env* env, int32_t slot, int32_t* buf, int32_t cap) {
    return guarded(env, [&] {
        if (slot < 0 || slot >= env->nSlots) throw Fail{-EINVAL, "slot out of range"};
        int pl;
        const int g = env->gameOfSlot(slot, &pl);
        const size_t sw = env->blockWords();
        std::vector<int32_t> s(sw);
        HIPCHK(hipStreamSynchronize(env->stream));
        HIPCHK(hipMemcpy(s.data(), env->d_state + (size_t)g * sw, sw * 4, hipMemcpyDeviceToHost));
        const std::vector<int32_t> d = canonicalDump(s.data(), env->CAP);
        if ((int)d.size() > cap) return -(int)d.size();
        std::memcpy(buf, d.data(), d.size() * 4);
        return (int)d.size();
    });
}

int mrts_utt_json(int32_t utt_version, int32_t conflict_policy, const char* utt_json, char* buf, int32_t cap) {
    return guardedCall([&] {
        const std::string j = uttToJson(utt_json ? uttFromJson(utt_json) : makeUtt(utt_version, conflict_policy));
        if (!buf || cap < (int32_t)j.size() + 1) return -((int)j.size() + 1);
        std::memcpy(buf, j.c_str(), j.size() + 1);
        return (int)j.size();
    });
}

static int readHeaderWord(mrts_env* env, int word, int32_t* out_per_slot) {
    const size_t sw = env->blockWords();
    HIPCHK(hipStreamSynchronize(env->stream));
    std::vector<int32_t> w((size_t)env->nGames);
    HIPCHK(hipMemcpy2D(w.data(), 4, env->d_state + word, sw * 4, 4, (size_t)env->nGames, hipMemcpyDeviceToHost));
    for (int s = 0; s < env->nSlots; s++) {
        int pl;
        out_per_slot[s] = w[(size_t)env->gameOfSlot(s, &pl)];
    }
    return 0;
}

int mrts_error_flags(mrts_env* env, uint32_t* flags) {
    return guarded(env, [&] { return readHeaderWord(env, H_ERR, (int32_t*)flags); });
}

int mrts_env_steps(mrts_env* env, int32_t* out) {
    return guarded(env, [&] { return readHeaderWord(env, H_STEPS, out); });
}

void mrts_destroy(mrts_env* env) {
    if (!env) return;
    (void)hipSetDevice(env->device);
    if (env->stream) (void)hipStreamSynchronize(env->stream);
    (void)hipFree(env->d_static);
    (void)hipFree(env->d_poPrev);
    (void)hipFree(env->d_prioTab);
    (void)hipFree(env->d_renderErr);
    (void)hipFree(env->d_packOverflow);
    (void)hipFree(env->d_obsPackCnt);
    (void)hipFree(env->d_bal);
    (void)hipFree(env->d_state);
    (void)hipFree(env->d_polPrev);
    (void)hipFree(env->d_pairs);
    (void)hipFree(env->d_rowsStage);
    (void)hipFree(env->d_masks32);
    (void)hipFree(env->d_copyPairs);
    (void)hipFree(env->d_eval);
    (void)hipFree(env->d_tmpl);
    (void)hipFree(env->d_tmplOff);
    (void)hipFree(env->d_gameKind);
    (void)hipFree(env->d_actions);
    (void)hipFree(env->d_players);
    (void)hipFree(env->d_obs);
    (void)hipFree(env->d_reward);
    (void)hipFree(env->d_done);
    (void)hipFree(env->d_masks);
    (void)hipHostFree(env->h_obs);
    (void)hipHostFree(env->h_masks);
    (void)hipHostFree(env->h_masks32);
    (void)hipHostFree(env->h_reward);
    (void)hipHostFree(env->h_done);
    if (env->stream) (void)hipStreamDestroy(env->stream);
    if (env->exStream) (void)hipStreamSynchronize(env->exStream);
    if (env->exComm) (void)g_rccl.commDestroy(env->exComm);
    if (env->exStream) (void)hipStreamDestroy(env->exStream);
    if (env->capExec) (void)hipGraphExecDestroy(env->capExec);
    if (env->capGraph) (void)hipGraphDestroy(env->capGraph);
    for (int b = 0; b < 2; b++) {
        if (env->exReady[b]) (void)hipEventDestroy(env->exReady[b]);
        if (env->exDone[b]) (void)hipEventDestroy(env->exDone[b]);
    }
    delete env;
}

// ---------------------------------------------------------------- state serialisation (checkpoint / interop)
static void readBlock(mrts_env* env, int g, std::vector<int32_t>& s) {
    const size_t sw = env->blockWords();
    s.resize(sw);
    HIPCHK(hipStreamSynchronize(env->stream));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(s.data(), env->d_state + (size_t)g * sw, sw * 4, hipMemcpyDeviceToHost));
}

int mrts_get_state_json(mrts_env* env, int32_t slot, char* buf, int32_t cap) {
    return guarded(env, [&] {
        if (slot < 0 || slot >= env->nSlots) throw Fail{-EINVAL, "slot out of range"};
        int pl;
        std::vector<int32_t> s;
        readBlock(env, env->gameOfSlot(slot, &pl), s);
        const std::string j = gameToJson(*env, s);
        if (!buf || cap < (int32_t)j.size() + 1) return -((int)j.size() + 1);
        std::memcpy(buf, j.c_str(), j.size() + 1);
        return (int)j.size();
    });
}

int mrts_set_state_json(mrts_env* env, int32_t slot, const char* json) {
    return guarded(env, [&] {
        if (!json || slot < 0 || slot >= env->nSlots) throw Fail{-EINVAL, "bad argument"};
        int pl;
        const int g = env->gameOfSlot(slot, &pl);
        std::vector<int32_t> s;
        readBlock(env, g, s);
        jsonToBlock(*env, json, s);
        // an injected state starts with fresh AIs: the LightRush memory of this game is cleared
        std::fill(s.begin() + stateWords(env->CAP, env->HW), s.end(), 0);
        env->noteValues(s.data());
        const size_t sw = s.size();
        HIPCHK(hipMemcpy(env->d_state + (size_t)g * sw, s.data(), sw * 4, hipMemcpyHostToDevice));
        env->invalidateWrites();
        return 0;
    });
}

// whole-handle checkpoint: a header + every game's state block (random streams, envSteps, kind included)
int64_t mrts_checkpoint_size(const mrts_env* env) {
    if (!env) return -EINVAL;
    return ckptSize(*env);
}

int mrts_checkpoint(mrts_env* env, void* buf, int64_t cap) {
    return guarded(env, [&] {
        if (!buf) throw Fail{-EINVAL, "null argument"};
        if (cap < ckptSize(*env)) throw Fail{-ENOSPC, "buffer too small"};
        const CkptHeader h = ckptHeader(*env);
        std::memcpy(buf, &h, sizeof(h));
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy((char*)buf + sizeof(h), env->d_state, (size_t)h.words * h.nGames * 4, hipMemcpyDeviceToHost));
        return 0;
    });
}

int mrts_restore(mrts_env* env, const void* buf, int64_t size) {
    return guarded(env, [&] {
        if (!buf) throw Fail{-EINVAL, "null argument"};
        checkCkpt(*env, buf, size);
        const char* blocks = (const char*)buf + sizeof(CkptHeader);
        const size_t words = env->blockWords();
        for (int g = 0; g < env->nGames; g++) env->noteValues((const int32_t*)blocks + (size_t)g * words);
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(env->d_state, blocks, words * env->nGames * 4, hipMemcpyHostToDevice));
        env->invalidateWrites();
        return 0;
    });
}

// ---------------------------------------------------------------- forward model
static void checkCopy(const mrts_env* dst, const mrts_env* src) {
    if (!dst->forwardModel) throw Fail{-EINVAL, "copy destination must be a forward-model handle"};
    // launchCopyGames writes destination blocks of stateWords: a forward model never has LightRush memory (mrts_create)
    if (dst->hasLightRush) throw Fail{-ENOTSUP, "copy destination carries LightRush memory"};
    if (src->H != dst->H || src->W != dst->W || src->CAP != dst->CAP) throw Fail{-EINVAL, "handles differ in map size"};
    if (std::memcmp(&src->utt, &dst->utt, sizeof(DevUtt)) != 0) throw Fail{-EINVAL, "handles differ in unit-type table"};
    if (src->device != dst->device) throw Fail{-EINVAL, "handles live on different devices"};
}

int mrts_copy_games_dev(mrts_env* dst, const mrts_env* src, const int32_t* d_pairs, int32_t n, void* stream) {
    return guarded(dst, [&] {
        if (!src) src = dst;
        checkCopy(dst, src);
        if (n < 0 || (n > 0 && !d_pairs)) throw Fail{-EINVAL, "bad pairs"};
        HIPCHK(hipSetDevice(dst->device));
        HIPCHK(launchCopyGames(dst->d_state, src->d_state, d_pairs, n, dst->nGames, src->nGames, dst->CAP, dst->HW,
                               (int)src->blockWords(), pickStream(dst, stream)));
        dst->lastObsPtr = nullptr;
        return 0;
    });
}

int mrts_copy_games(mrts_env* dst, const mrts_env* src, const int32_t* pairs, int32_t n) {
    return guarded(dst, [&] {
        if (!src) src = dst;
        checkCopy(dst, src);
        if (n < 0 || (n > 0 && !pairs)) throw Fail{-EINVAL, "bad pairs"};
        std::vector<char> isDst((size_t)dst->nGames, 0), isSrc((size_t)src->nGames, 0);
        for (int i = 0; i < n; i++) {
            const int d = pairs[2 * i], s = pairs[2 * i + 1];
            if (d < 0 || d >= dst->nGames || s < 0 || s >= src->nGames) throw Fail{-EINVAL, "game index out of range"};
            if (isDst[(size_t)d]) throw Fail{-EINVAL, "a destination game appears twice"};
            isDst[(size_t)d] = 1;
            isSrc[(size_t)s] = 1;
        }
        if (src == dst)
            for (int g = 0; g < dst->nGames; g++)
                if (isDst[(size_t)g] && isSrc[(size_t)g]) throw Fail{-EINVAL, "a game is both a source and a destination"};
        if (n == 0) return 0;
        HIPCHK(hipSetDevice(dst->device));
        HIPCHK(hipStreamSynchronize(src->stream));
        if (n > dst->copyPairsCap) {
            HIPCHK(hipStreamSynchronize(dst->stream));
            (void)hipFree(dst->d_copyPairs);
            dst->d_copyPairs = nullptr;
            HIPCHK(hipMalloc(&dst->d_copyPairs, (size_t)n * 2 * 4));
            dst->copyPairsCap = n;
        }
        HIPCHK(hipMemcpyAsync(dst->d_copyPairs, pairs, (size_t)n * 2 * 4, hipMemcpyHostToDevice, dst->stream));
        HIPCHK(launchCopyGames(dst->d_state, src->d_state, dst->d_copyPairs, n, dst->nGames, src->nGames, dst->CAP,
                               dst->HW, (int)src->blockWords(), dst->stream));
        dst->lastObsPtr = nullptr;
        HIPCHK(hipStreamSynchronize(dst->stream));
        return 0;
    });
}

int mrts_playout_dev(mrts_env* env, int32_t horizon, void* stream) {
    return guarded(env, [&] {
        if (!env->forwardModel) throw Fail{-EINVAL, "not a forward-model handle"};
        if (horizon < -MRTS_MAX_HORIZON || horizon > MRTS_MAX_HORIZON) throw Fail{-EINVAL, "horizon out of range"};
        HIPCHK(hipSetDevice(env->device));
        KDyn D = mrts_env::noArgs();
        D.horizon = horizon;
        HIPCHK(env->launch(MODE_PLAYOUT, D, pickStream(env, stream)));
        env->lastObsPtr = nullptr;
        return 0;
    });
}

int mrts_playout(mrts_env* env, int32_t horizon) {
    return guarded(env, [&] {
        int r = mrts_playout_dev(env, horizon, env->stream);
        if (r) return r;
        HIPCHK(hipStreamSynchronize(env->stream));
        checkFlagsAfter(env);
        return 0;
    });
}

int mrts_trace_step(mrts_env* env, const int32_t* pairs, int32_t n_pairs, const int32_t* until, int32_t* out,
                    int32_t generic) {
    return guarded(env, [&] {
        if (!env->forwardModel) throw Fail{-EINVAL, "not a forward-model handle"};
        if (!until || (n_pairs > 0 && !pairs)) throw Fail{-EINVAL, "null argument"};
        if (n_pairs < 0 || (size_t)n_pairs * env->nGames * 8 >= ((size_t)1 << 31)) throw Fail{-EINVAL, "bad n_pairs"};
        const size_t nr = (size_t)env->nGames * n_pairs;
        for (size_t i = 0; i < nr; i++) {  // what Java could not construct (TraceEntry.fromXML, UnitAction(...))
            const int32_t* r = pairs + 8 * i;
            if (r[0] < -1 || r[0] > 1) throw Fail{-EINVAL, "pair player must be 0, 1 or -1 (padding)"};
            if (r[0] < 0) continue;
            if (r[3] == 4 && (r[7] < 0 || r[7] >= env->utt.ntypes)) throw Fail{-EINVAL, "PRODUCE of an unknown unit type"};
            if (r[4] < -32768 || r[4] > 32767) throw Fail{-EINVAL, "parameter out of the int16 range"};
        }
        for (int g = 0; g < env->nGames; g++)
            if (until[g] < 0 || until[g] > (1 << 30)) throw Fail{-EINVAL, "until out of range"};
        HIPCHK(hipSetDevice(env->device));
        HIPCHK(hipStreamSynchronize(env->stream));
        const size_t need = nr * 8 + 2 * (size_t)env->nGames;
        if (need > env->rowsStageInts) {
            (void)hipFree(env->d_rowsStage);
            env->d_rowsStage = nullptr;
            HIPCHK(hipMalloc(&env->d_rowsStage, need * 4));
            env->rowsStageInts = need;
        }
        int32_t* d_until = env->d_rowsStage + nr * 8;
        if (nr) HIPCHK(hipMemcpyAsync(env->d_rowsStage, pairs, nr * 8 * 4, hipMemcpyHostToDevice, env->stream));
        HIPCHK(hipMemcpyAsync(d_until, until, (size_t)env->nGames * 4, hipMemcpyHostToDevice, env->stream));
        KDyn D = mrts_env::noArgs();
        D.rows = env->d_rowsStage;
        D.n_rows = n_pairs;
        D.trace_until = d_until;
        D.trace_out = d_until + env->nGames;
        D.trace_generic = generic ? 1 : 0;
        HIPCHK(env->launch(MODE_TRACE, D, env->stream));
        env->lastObsPtr = nullptr;
        env->fusedActions = nullptr;
        std::vector<int32_t> o((size_t)env->nGames);
        HIPCHK(hipMemcpyAsync(o.data(), D.trace_out, (size_t)env->nGames * 4, hipMemcpyDeviceToHost, env->stream));
        HIPCHK(hipStreamSynchronize(env->stream));
        if (out) std::memcpy(out, o.data(), o.size() * 4);
        checkFlagsAfter(env);
        return 0;
    });
}

int mrts_evaluate_dev(mrts_env* env, int32_t maxplayer, float* d_out, void* stream) {
    return guarded(env, [&] {
        if (!d_out) throw Fail{-EINVAL, "null argument"};
        if (maxplayer != 0 && maxplayer != 1) throw Fail{-EINVAL, "maxplayer must be 0 or 1"};
        HIPCHK(hipSetDevice(env->device));
        HIPCHK(launchEvaluate(env->hstatic, env->d_static, maxplayer, d_out, pickStream(env, stream)));
        return 0;
    });
}

int mrts_evaluate(mrts_env* env, int32_t maxplayer, float* out) {
    return guarded(env, [&] {
        if (!out) throw Fail{-EINVAL, "null argument"};
        if (!env->d_eval) HIPCHK(hipMalloc(&env->d_eval, (size_t)env->nGames * 4));
        int r = mrts_evaluate_dev(env, maxplayer, env->d_eval, env->stream);
        if (r) return r;
        HIPCHK(hipMemcpyAsync(out, env->d_eval, (size_t)env->nGames * 4, hipMemcpyDeviceToHost, env->stream));
        HIPCHK(hipStreamSynchronize(env->stream));
        return 0;
    });
}

#ifdef MRTS_LANE_AUDIT
// diagnostic build only: the cross-lane read audit (tests/test_zz_lane_audit.py); synchronises the device
int mrts_lane_audit(int32_t* out, int reset) {
    if (hipDeviceSynchronize() != hipSuccess) return -EIO;
    return mrts::laneAudit(out, reset) == hipSuccess ? 0 : -EIO;
}
// the negative control: one launch whose readlane reads an inactive lane (the audit must report it)
int mrts_lane_audit_probe(void) {
    int32_t* d = nullptr;
    if (hipMalloc(&d, 64 * sizeof(int32_t)) != hipSuccess) return -ENOMEM;
    const hipError_t e = mrts::laneAuditProbe(d);
    const hipError_t s = hipDeviceSynchronize();
    (void)hipFree(d);
    return e == hipSuccess && s == hipSuccess ? 0 : -EIO;
}
#endif
#ifdef MRTS_ABLATE
#include "mrts_ablate.h"
// diagnostic build only: g_ablate (tools/ablate_price.py), bit b = the row of mrts_ablate.h with that bit
int mrts_set_ablate(unsigned long long v) { return mrts::setAblate(v) == hipSuccess ? 0 : -EIO; }
// that table, row by row: the row whose bit is `bit` — its enum name, kind ("AGAIN" / "SKIP" / "COUNT"), the name the
// tools print and its name on the steady instance (NULL where it is the same) — or -ENOENT when no row has that bit
int mrts_ablate_phase(int bit, const char** enum_name, const char** kind, const char** name, const char** steady_name) {
    static const struct { int bit; const char *en, *kind, *name, *steady; } rows[] = {
#define X(n, bit, kind, name, steadyName) {bit, "AB_" #n, #kind, name, steadyName},
        MRTS_AB_PHASES(X)
#undef X
    };
    for (const auto& r : rows)
        if (r.bit == bit) {
            *enum_name = r.en, *kind = r.kind, *name = r.name, *steady_name = r.steady;
            return 0;
        }
    return -ENOENT;
}
int mrts_get_dbg(unsigned long long* out, int reset) { return mrts::getDbg(out, reset) == hipSuccess ? 0 : -EIO; }
#endif
#ifdef MRTS_PHASE_TIMING
// diagnostic build only: per-phase cycle sums of k_env (tools/phase_timing.py)
int mrts_phase_times(unsigned long long* out, int reset) { return mrts::phaseTimes(out, reset) == hipSuccess ? 0 : -EIO; }
int mrts_phase_spans(unsigned long long* out, int n) { return mrts::phaseSpans(out, n) == hipSuccess ? 0 : -EIO; }
#endif
}  // extern "C"
