// mrts_launch.h — the one declaration of everything mrts_host.cpp calls in the .hip units (mrts_kernels.hip: the
// step kernel; mrts_policy.hip: the random policies and the masked head; mrts_aux.hip: renderers, packed observation
// rows, copies, evaluation).
// The host and every unit include it, so a definition that drifts from its declaration fails to compile.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "mrts_internal.h"

namespace mrts {
// ---- mrts_kernels.hip
size_t ldsBytes(int HW, int W, int CAP, int po);
size_t lrLdsBytes(int HW, int W, int CAP);
// a handle's dynamic LDS: the game's own, or with a LightRush game its area (lrLdsBytes) from the next 16-byte
// boundary on — ldsLightRushOff, KStatic.bot_lds
size_t ldsLightRushOff(int HW, int W, int CAP, int po);
size_t handleLdsBytes(int HW, int W, int CAP, int po, bool lightRush);
hipError_t launchEnv(int mode, const KStatic& hs, const KStatic* ds, const KDyn& D, hipStream_t stream, hipEvent_t e0 = nullptr,
                     hipEvent_t e1 = nullptr);
bool envIterable(const KStatic& hs);
hipError_t prepareLds(size_t bytes);
#ifdef MRTS_LANE_AUDIT
hipError_t laneAudit(int32_t* out, int reset);
hipError_t laneAuditProbe(int32_t* scratch);
// every unit's own record (its g_laneAudit, mrts_device.h), merged into out[256]; UNIT = the unit's MRTS_UNIT
template <int UNIT>
hipError_t laneAuditUnit(int32_t* out, int reset);
template <>
hipError_t laneAuditUnit<0>(int32_t* out, int reset);
template <>
hipError_t laneAuditUnit<1>(int32_t* out, int reset);
template <>
hipError_t laneAuditUnit<2>(int32_t* out, int reset);
#endif
#ifdef MRTS_ABLATE
hipError_t setAblate(uint64_t v);
hipError_t getDbg(unsigned long long* out, int reset);
#endif
#ifdef MRTS_PHASE_TIMING
hipError_t phaseTimes(unsigned long long* out, int reset);
hipError_t phaseSpans(unsigned long long* out, int n);
#endif
// ---- mrts_policy.hip
hipError_t launchPolicyUniform(int32_t* actions, int n_slots, int HW, int ntypes, int natt, uint64_t seed, uint32_t step,
                               uint32_t slot_base, hipStream_t stream);
hipError_t launchPolicy(const PolicyParams& Q, hipStream_t stream, bool* prevWritten);
hipError_t launchHead(int mode, const HeadParams& Q, hipStream_t stream);
hipError_t launchHeadPacked(int mode, const HeadPackedParams& P, hipStream_t stream);
// ---- mrts_aux.hip
hipError_t launchWiden(const uint8_t* in, int32_t* out, size_t n, hipStream_t stream);
hipError_t launchOneHot(const int32_t* obs, uint8_t* out, int n_slots, int HW, int C, int ntypes, hipStream_t stream);
hipError_t launchCopyGames(int32_t* dst, const int32_t* src, const int32_t* pairs, int n, int n_dst, int n_src,
                           int CAP, int HW, int src_words, hipStream_t stream);
hipError_t launchEvaluate(const KStatic& hs, const KStatic* ds, int maxplayer, float* out, hipStream_t stream);
hipError_t launchRenderRecords(const KStatic& hs, const KStatic* ds, const uint32_t* rec, int units, int n_ranks,
                               int64_t rank_stride, void* out, int out_bytes, int32_t* err, hipStream_t stream);
hipError_t launchRenderRecordsOneHot(const KStatic& hs, const KStatic* ds, const uint32_t* rec, int64_t rec_words, int n_ranks,
                                     int units, int64_t rank_stride, const int32_t* sel, const int64_t* step_off, int n_sel,
                                     uint8_t* out, int32_t* err, hipStream_t stream);
// mode: OBS_PACK / OBS_UNPACK / OBS_ONEHOT (the one-hot table is filled here from P.C and ntypes)
hipError_t launchObsPacked(int mode, ObsPackParams P, int ntypes, hipStream_t stream);
}  // namespace mrts
