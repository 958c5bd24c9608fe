// mrts_hostdata.h — the host runtime's data work that needs no GPU: unit-type tables and their JSON, the XML map
// reader, state block <-> GameState JSON, the canonical state dump, the checkpoint header and the configuration half
// of mrts_create.  Plain C++17 on mrts_internal.h (no HIP header): mrts_host.cpp calls it behind a handle, the
// internal probes and hostcheck.cpp call it without one.
#pragma once
#include <stdint.h>

#include <cerrno>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/mrts.h"
#include "mrts_internal.h"

namespace mrts {

// an entry point's refusal: the error code it returns and the text mrts_last_error() then holds
struct Fail {
    int code;
    std::string msg;
};
// The one boundary between C++ and a C caller: body()'s value, or for a Fail its code, for an allocation failure
// -ENOMEM and for any other std::exception -EINVAL, with the text in err.  Nothing is thrown across it.
template <class F>
int guardCall(std::string& err, F&& body) {
    try {
        return body();
    } catch (const Fail& f) {
        err = f.msg;
        return f.code;
    } catch (const std::bad_alloc&) {
        err = "out of memory";
        return -ENOMEM;
    } catch (const std::exception& e) {
        err = e.what();
        return -EINVAL;
    }
}

// ------------------------------------------------------------------ unit type tables
// The device table (DevUtt) plus what only the host needs: names (map loading, toJSON),
// returnTime and producedBy (toJSON only; RETURN lasts moveTime, UnitAction.java:321-322).
struct UttInfo {
    DevUtt dev;
    std::vector<std::string> names;
    std::vector<int> returnT;
    std::vector<std::vector<int>> producedBy;
    int typeOf(const std::string& n) const {
        for (size_t t = 0; t < names.size(); t++)
            if (names[t] == n) return (int)t;
        return -1;
    }
};
UttInfo makeUtt(int version, int crs);
UttInfo uttFromJson(const std::string& text);
std::string uttToJson(const UttInfo& I);
uint32_t uttHash(const DevUtt& u);

// ------------------------------------------------------------------ XML map reader
struct MapDef {
    int W = 0, H = 0;
    std::vector<uint8_t> terrain;
    int res[2] = {0, 0};
    struct U { int type, player, x, y, res, hp; long long id; };
    std::vector<U> units;
};
MapDef parseMapText(const std::string& x, const std::string& path, const UttInfo& utt);  // path: for the messages
MapDef parseMap(const std::string& path, const UttInfo& utt);

// ------------------------------------------------------------------ state blocks
// what the converters need to know of a handle
struct StateShape {
    int H = 0, W = 0, HW = 0, CAP = 0;
    int maxUnits = 0;  // live-unit bound (H*W unless mrts_config.max_units)
    UttInfo uttInfo;
};
std::string gameToJson(const StateShape& env, const std::vector<int32_t>& s);
void jsonToBlock(const StateShape& env, const std::string& text, std::vector<int32_t>& s);
// the canonical dump of mrts_get_state (include/mrts.h) of state block s
std::vector<int32_t> canonicalDump(const int32_t* s, int CAP);
// every live unit's hp and resources lie in 0..255 (what the byte renders can show)
bool valuesFitBytes(const int32_t* s, int CAP);

// ------------------------------------------------------------------ a handle's configuration
// what mrts_create settles before its first device call, kept by the handle for its lifetime
struct HandleConfig : StateShape {
    int device = 0;
    int C = 6, K = 79;
    int nSlots = 0, nGames = 0, nSpGames = 0, maxSteps = 0, partialObs = 0;
    int forwardModel = 0;  // games advance through mrts_playout* only (GT_PLAYOUT)
    int botOnly = 0;       // the bot-only client (ai1_kinds): reward / done only, no observation or masks
    // native LightRush: the handle has a LightRush game, so every state block carries the bot's memory
    // (mrts_internal.h botWords) after its stateWords; botTypes = the types named Base, Barracks, Worker, Light
    int hasLightRush = 0;
    uint32_t botTypes = 0;
    size_t blockWords() const { return (size_t)stateWords(CAP, HW) + (hasLightRush ? (size_t)botWords(CAP) : 0); }
    uint32_t slotIdBase = 0;
    DevUtt utt;
    std::vector<int> tmplOffHost;
    uint32_t cfgHash = 0;  // game kinds, map templates, max_steps, reward kinds, PO (checkpoint compatibility)
    std::vector<int32_t> gameKindHost;
    int maskDelta = 0;
    int obsImg = 0;  // KDyn.obs_img: every observation value fits a byte
    std::vector<int32_t> rewardKinds{RF_WINLOSS};  // a_rfs
};
// the configuration half of mrts_create: everything it validates and derives without a device
struct CreatePlan {
    HandleConfig cfg;
    int mostMapUnits = 0;           // the largest unit count of a map (checked against max_units after the LDS size)
    std::vector<int32_t> blob;      // the map templates (mrts_internal.h "map templates")
    std::vector<int32_t> rngWords;  // per game H_RNG_CANCEL .. H_RNG_SAMPLER + 1: the java.util.Random seeds
};
CreatePlan planCreate(const mrts_config* cfg);

// ------------------------------------------------------------------ whole-handle checkpoint
// a header + every game's state block (random streams, envSteps, kind included)
struct CkptHeader {
    char magic[8];
    int32_t version, H, W, CAP, nGames, nSpGames, words;
    uint32_t uttHash;
    uint32_t cfgHash;  // HandleConfig::cfgHash: game kinds (opponents), map templates, max_steps, reward kinds, PO
    int32_t pad_;
};
CkptHeader ckptHeader(const HandleConfig& c);
inline int64_t ckptSize(const HandleConfig& c) { return (int64_t)sizeof(CkptHeader) + (int64_t)c.blockWords() * c.nGames * 4; }
// the checks of mrts_restore on a checkpoint of `size` bytes at buf; throws Fail
void checkCkpt(const HandleConfig& c, const void* buf, int64_t size);

// ------------------------------------------------------------------ packed observation rows
// The argument checks of mrts_obs_pack_dev / _unpack_dev / _onehot_packed_dev (include/mrts.h), without a device:
// the shape fields of the kernels' parameters for n_rows rows at `cap`, then the buffers; each throws Fail.
ObsPackParams obsPackShape(const HandleConfig& c, int32_t n_rows, int32_t cap);
void obsPackBuffers(ObsPackParams& P, const int32_t* d_obs, uint32_t* d_out);
// out_align: 4 (the int32 planes) or 16 (the one-hot bytes)
void obsPackedSource(ObsPackParams& P, const uint32_t* d_packed, int32_t n_packed, const int32_t* d_index, const void* d_out,
                     int out_align);

}  // namespace mrts
