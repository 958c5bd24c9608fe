// mrts_hostdata.cpp — see mrts_hostdata.h.  Compiled by hipcc into libmrts.so like the other units, and by the host
// compiler alone for `make hostcheck` (hostcheck.cpp, under the address and undefined-behaviour sanitizers).
#include "mrts_hostdata.h"

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>

#include "mrts_json.hpp"

namespace mrts {

static const char* kTypeNames[7] = {"Resource", "Base", "Barracks", "Worker", "Light", "Heavy", "Ranged"};

// the reward functions' type-name tests as flag bits; K and the attack radius from the table
static void finishUtt(UttInfo& I) {
    DevUtt& u = I.dev;
    for (int t = 0; t < u.ntypes; t++) {
        const std::string& n = I.names[(size_t)t];
        if (n == "Resource") u.flags[t] |= N_RESOURCE;
        if (n == "Base") u.flags[t] |= N_BASE | N_BUILDING;
        if (n == "Barracks") u.flags[t] |= N_BUILDING;
        if (n == "Worker") u.flags[t] |= N_WORKER;
        if (n == "Light" || n == "Heavy" || n == "Ranged") u.flags[t] |= N_COMBAT;
    }
    int maxRange = 0;  // UnitTypeTable.getMaxAttackRange (:341-349)
    for (int t = 0; t < u.ntypes; t++) maxRange = std::max(maxRange, u.range[t]);
    u.maxAttackRadius = 2 * maxRange + 1;
    u.K = 1 + 6 + 4 + 4 + 4 + 4 + u.ntypes + u.maxAttackRadius * u.maxAttackRadius;
    u.mtAttack1 = u.mtAttackFar = u.mtHarvest = u.mtMove = u.mtResource = u.mtStockpile = 0;
    uint64_t prod = 0;
    for (int t = 0; t < u.ntypes; t++) {  // the mask tables (Game::maskTables)
        const uint32_t f = u.flags[t], b = 1u << t;
        if ((f & F_ATTACK) && u.range[t] == 1) u.mtAttack1 |= b;
        if ((f & F_ATTACK) && u.range[t] > 1) u.mtAttackFar |= b;
        if (f & F_HARVEST) u.mtHarvest |= b;
        if (f & F_MOVE) u.mtMove |= b;
        if (f & F_RESOURCE) u.mtResource |= b;
        if (f & F_STOCKPILE) u.mtStockpile |= b;
        for (int i = 0; i < u.nprod[t]; i++) prod |= (uint64_t)1 << (8 * t + u.prod[t][i]);
    }
    u.mtProdLo = (uint32_t)prod;
    u.mtProdHi = (uint32_t)(prod >> 32);
    u.maxSight = 0;
    for (int t = 0; t < u.ntypes; t++) {  // integer floor(sqrt(r^2 - dy^2)): the cells dx^2 + dy^2 <= r^2
        const int r = u.sight[t];
        u.maxSight = std::max(u.maxSight, r);
        u.diskLo[t] = u.diskHi[t] = 0;
        if (r > 15) continue;  // painted with the sqrt form
        for (int dy = 0; dy <= r; dy++) {
            int w = 0;
            while ((w + 1) * (w + 1) + dy * dy <= r * r) w++;
            if (dy < 8) u.diskLo[t] |= (uint32_t)w << (4 * dy);
            else u.diskHi[t] |= (uint32_t)w << (4 * (dy - 8));
        }
    }
}

// new UnitTypeTable(version, crs) — reference src/rts/units/UnitTypeTable.java:104-289
UttInfo makeUtt(int version, int crs) {
    if (version < 1 || version > 3) throw Fail{-EINVAL, "utt_version must be 1, 2 or 3"};
    if (crs < 1 || crs > 3) throw Fail{-EINVAL, "conflict_policy must be 1, 2 or 3"};
    DevUtt u;
    std::memset(&u, 0, sizeof(u));
    u.ntypes = 7;
    for (int t = 0; t < 7; t++) {  // UnitType defaults (rts/units/UnitType.java:33-100)
        u.cost[t] = 1;
        u.hp[t] = 1;
        u.minD[t] = u.maxD[t] = 1;
        u.range[t] = 1;
        u.produceT[t] = u.moveT[t] = u.attackT[t] = u.harvestT[t] = 10;
        u.harvestAmt[t] = 1;
        u.sight[t] = 4;
        u.flags[t] = F_MOVE | F_ATTACK;
    }
    const bool v1 = version == 1, v2 = version == 2, v3 = version == 3;
    // Resource
    u.flags[0] = F_RESOURCE;
    u.sight[0] = 0;
    // Base
    u.cost[1] = 10; u.hp[1] = 10;
    if (v1) u.produceT[1] = 250;
    else if (v2) u.produceT[1] = 200;
    u.flags[1] = F_STOCKPILE;
    u.sight[1] = 5;
    // Barracks
    u.cost[2] = 5; u.hp[2] = 4;
    u.produceT[2] = v1 ? 200 : 100;
    u.flags[2] = 0;
    u.sight[2] = 3;
    // Worker
    u.cost[3] = 1; u.hp[3] = 1;
    if (v3) { u.minD[3] = 0; u.maxD[3] = 2; }
    u.range[3] = 1; u.produceT[3] = 50; u.moveT[3] = 10; u.attackT[3] = 5; u.harvestT[3] = 20;
    u.flags[3] = F_HARVEST | F_MOVE | F_ATTACK;
    u.sight[3] = 3;
    // Light
    u.cost[4] = 2; u.hp[4] = 4;
    if (v3) { u.minD[4] = 1; u.maxD[4] = 3; } else { u.minD[4] = u.maxD[4] = 2; }
    u.produceT[4] = 80; u.moveT[4] = 8; u.attackT[4] = 5;
    u.flags[4] = F_MOVE | F_ATTACK;
    u.sight[4] = 2;
    // Heavy
    if (v3) { u.minD[5] = 0; u.maxD[5] = 6; } else { u.minD[5] = u.maxD[5] = 4; }
    u.produceT[5] = 120;
    if (v1) { u.moveT[5] = 12; u.hp[5] = 4; u.cost[5] = 2; } else { u.moveT[5] = 10; u.hp[5] = 8; u.cost[5] = 3; }
    u.attackT[5] = 5;
    u.flags[5] = F_MOVE | F_ATTACK;
    u.sight[5] = 2;
    // Ranged
    u.cost[6] = 2; u.hp[6] = 1;
    if (v3) { u.minD[6] = 1; u.maxD[6] = 2; }
    u.range[6] = 3; u.produceT[6] = 100; u.moveT[6] = 10; u.attackT[6] = 5;
    u.flags[6] = F_MOVE | F_ATTACK;
    u.sight[6] = 3;
    // produces lists, in declaration order (:283-288)
    u.nprod[1] = 1; u.prod[1][0] = 3;
    u.nprod[2] = 3; u.prod[2][0] = 4; u.prod[2][1] = 5; u.prod[2][2] = 6;
    u.nprod[3] = 2; u.prod[3][0] = 1; u.prod[3][1] = 2;
    u.crs = crs;
    UttInfo I;
    I.dev = u;
    I.names.assign(kTypeNames, kTypeNames + 7);
    I.returnT.assign(7, 10);
    // producedBy in the order of the produces() calls (:283-288): type order here
    I.producedBy.assign(7, {});
    for (int t = 0; t < 7; t++)
        for (int i = 0; i < u.nprod[t]; i++) I.producedBy[(size_t)u.prod[t][i]].push_back(t);
    finishUtt(I);
    return I;
}

// UnitTypeTable.fromJSON (:414-433) + UnitType.createStub / updateFromJSON
// (UnitType.java:156-161, 217-248), including its quirks: harvestTime is read from "produceTime",
// returnTime is not read, and absent members take updateFromJSON's defaults (harvestAmount and sightRadius default to 10,
// canMove / canAttack to false).  Limits of this build: <= 8 types, type IDs equal to their list
// positions, <= 4 produced types, attack range <= 3 (K <= 80 mask slots: an idle unit's mask is
// parked as 80 bits in its free assignment words), hp in int16, positive durations; every produced /
// producedBy name must exist.
UttInfo uttFromJson(const std::string& text) {
    mjson::Value o;
    try {
        o = mjson::parse(text);
    } catch (const std::runtime_error& e) {
        throw Fail{-EINVAL, std::string("utt_json: ") + e.what()};
    }
    try {
        if (o.kind != mjson::Value::OBJ) throw Fail{-EINVAL, "utt_json: not an object"};
        const int crs = o.getInt("moveConflictResolutionStrategy", 1);
        if (crs < 1 || crs > 3) throw Fail{-ENOTSUP, "utt_json: moveConflictResolutionStrategy must be 1, 2 or 3"};
        const mjson::Value& a = o.at("unitTypes");
        if (a.kind != mjson::Value::ARR) throw Fail{-EINVAL, "utt_json: unitTypes is not an array"};
        const int n = (int)a.arr.size();
        if (n < 1 || n > MAX_TYPES) throw Fail{-ENOTSUP, "utt_json: 1..8 unit types supported"};
        UttInfo I;
        DevUtt& u = I.dev;
        std::memset(&u, 0, sizeof(u));
        u.ntypes = n;
        u.crs = crs;
        for (int t = 0; t < n; t++) {  // createStub: ID and name
            const mjson::Value& ut = a.arr[(size_t)t];
            if (ut.getInt("ID", -1) != t) throw Fail{-ENOTSUP, "utt_json: type IDs must equal their list positions"};
            I.names.push_back(ut.getString("name", ""));
        }
        I.returnT.assign((size_t)n, 10);
        I.producedBy.assign((size_t)n, {});
        auto lookup = [&](const mjson::Value& v) {
            if (v.kind != mjson::Value::STR) throw Fail{-EINVAL, "utt_json: type names must be strings"};
            const int k = I.typeOf(v.s);
            if (k < 0) throw Fail{-EINVAL, "utt_json: unknown unit type " + v.s};
            return k;
        };
        for (int t = 0; t < n; t++) {  // updateFromJSON
            const mjson::Value& ut = a.arr[(size_t)t];
            u.cost[t] = ut.getInt("cost", 1);
            u.hp[t] = ut.getInt("hp", 1);
            u.minD[t] = ut.getInt("minDamage", 1);
            u.maxD[t] = ut.getInt("maxDamage", 1);
            u.range[t] = ut.getInt("attackRange", 1);
            u.produceT[t] = ut.getInt("produceTime", 10);
            u.moveT[t] = ut.getInt("moveTime", 10);
            u.attackT[t] = ut.getInt("attackTime", 10);
            u.harvestT[t] = ut.getInt("produceTime", 10);  // sic (UnitType.java:227)
            u.harvestAmt[t] = ut.getInt("harvestAmount", 10);
            u.sight[t] = ut.getInt("sightRadius", 10);
            uint32_t f = 0;
            if (ut.getBool("isResource", false)) f |= F_RESOURCE;
            if (ut.getBool("isStockpile", false)) f |= F_STOCKPILE;
            if (ut.getBool("canHarvest", false)) f |= F_HARVEST;
            if (ut.getBool("canMove", false)) f |= F_MOVE;
            if (ut.getBool("canAttack", false)) f |= F_ATTACK;
            u.flags[t] = f;
            const mjson::Value& pr = ut.at("produces");
            if (pr.kind != mjson::Value::ARR || pr.arr.size() > (size_t)MAX_PRODUCES)
                throw Fail{-ENOTSUP, "utt_json: at most 4 produced types per type"};
            u.nprod[t] = (int)pr.arr.size();
            for (size_t i = 0; i < pr.arr.size(); i++) u.prod[t][i] = lookup(pr.arr[i]);
            const mjson::Value& pb = ut.at("producedBy");
            if (pb.kind != mjson::Value::ARR) throw Fail{-EINVAL, "utt_json: producedBy is not an array"};
            for (auto& v : pb.arr) I.producedBy[(size_t)t].push_back(lookup(v));
            if (u.hp[t] < 1 || u.hp[t] > 32767 || u.cost[t] < 0 || u.cost[t] > 32767 || u.minD[t] < 0 ||
                u.maxD[t] < u.minD[t] || u.maxD[t] > 32767 || u.range[t] < 1 || u.range[t] > 3 ||
                u.produceT[t] < 1 || u.moveT[t] < 1 || u.attackT[t] < 1 || u.harvestT[t] < 1 ||
                u.harvestAmt[t] < 0 || u.harvestAmt[t] > 32767 || u.sight[t] < 0 || u.sight[t] > 64)
                throw Fail{-ENOTSUP, "utt_json: a value of type " + I.names[(size_t)t] + " is outside this build's limits"};
        }
        finishUtt(I);
        return I;
    } catch (const std::runtime_error& e) {
        throw Fail{-EINVAL, std::string("utt_json: ") + e.what()};
    }
}

// UnitTypeTable.toJSON (:372-383) + UnitType.toJSON (UnitType.java:299-343), byte for byte
std::string uttToJson(const UttInfo& I) {
    const DevUtt& u = I.dev;
    auto b = [](bool v) { return v ? "true" : "false"; };
    std::ostringstream w;
    w << "{\"moveConflictResolutionStrategy\":" << u.crs << ",\"unitTypes\":[";
    for (int t = 0; t < u.ntypes; t++) {
        if (t) w << ", ";
        const uint32_t f = u.flags[t];
        w << "{\"ID\":" << t << ", \"name\":\"" << I.names[(size_t)t] << "\", \"cost\":" << u.cost[t] << ", \"hp\":" << u.hp[t]
          << ", \"minDamage\":" << u.minD[t] << ", \"maxDamage\":" << u.maxD[t] << ", \"attackRange\":" << u.range[t]
          << ", \"produceTime\":" << u.produceT[t] << ", \"moveTime\":" << u.moveT[t] << ", \"attackTime\":" << u.attackT[t]
          << ", \"harvestTime\":" << u.harvestT[t] << ", \"returnTime\":" << I.returnT[(size_t)t]
          << ", \"harvestAmount\":" << u.harvestAmt[t] << ", \"sightRadius\":" << u.sight[t]
          << ", \"isResource\":" << b(f & F_RESOURCE) << ", \"isStockpile\":" << b(f & F_STOCKPILE)
          << ", \"canHarvest\":" << b(f & F_HARVEST) << ", \"canMove\":" << b(f & F_MOVE)
          << ", \"canAttack\":" << b(f & F_ATTACK) << ", \"produces\":[";
        for (int i = 0; i < u.nprod[t]; i++) w << (i ? ", " : "") << "\"" << I.names[(size_t)u.prod[t][i]] << "\"";
        w << "], \"producedBy\":[";
        for (size_t i = 0; i < I.producedBy[(size_t)t].size(); i++)
            w << (i ? ", " : "") << "\"" << I.names[(size_t)I.producedBy[(size_t)t][i]] << "\"";
        w << "]}";
    }
    w << "]}";
    return w.str();
}

uint32_t uttHash(const DevUtt& u) {
    uint32_t h = 2166136261u;
    const uint8_t* p = (const uint8_t*)&u;
    for (size_t i = 0; i < sizeof(DevUtt); i++) h = (h ^ p[i]) * 16777619u;
    return h;
}

// ------------------------------------------------------------------ XML map reader
// rts/PhysicalGameState.java:700-726 (fromXML), :765-777 + :577-607 (terrain, raw or A/B RLE),
// rts/units/Unit.java:597-620 (unit attributes).
static std::string attrOf(const std::string& tag, const char* name) {
    const std::string key(name);
    size_t p = 0;
    while ((p = tag.find(key, p)) != std::string::npos) {
        const bool start = p == 0 || isspace((unsigned char)tag[p - 1]);
        size_t q = p + key.size();
        while (q < tag.size() && isspace((unsigned char)tag[q])) q++;
        if (start && q < tag.size() && tag[q] == '=') {
            q++;
            while (q < tag.size() && isspace((unsigned char)tag[q])) q++;
            if (q < tag.size() && tag[q] == '"') {
                const size_t e = tag.find('"', q + 1);
                return tag.substr(q + 1, e - q - 1);
            }
        }
        p += key.size();
    }
    throw Fail{-EINVAL, std::string("map: missing attribute ") + name};
}

static int toInt(const std::string& s) {
    try {
        return std::stoi(s);
    } catch (...) {
        throw Fail{-EINVAL, "map: bad integer '" + s + "'"};
    }
}

// terrain text, raw digits or the A/B run-length form (PhysicalGameState.java:577-607,765-777)
static std::vector<int> decodeTerrain(const std::string& ts, int HW) {
    std::vector<int> terr;
    if (ts.find('A') != std::string::npos || ts.find('B') != std::string::npos) {
        std::string counter;
        for (char ch : ts) {
            if (ch == 'A' || ch == 'B') {
                if (!counter.empty()) {
                    const int n = toInt(counter);
                    if (terr.empty() || n < 1 || n > HW) throw Fail{-EINVAL, "terrain: bad run length"};
                    for (int i = 0; i < n - 1; i++) terr.push_back(terr.back());
                    counter.clear();
                }
                terr.push_back(ch == 'A' ? 0 : 1);
            } else if (!isspace((unsigned char)ch)) {
                counter.push_back(ch);
            }
        }
        if (!counter.empty()) {
            const int n = toInt(counter);
            if (terr.empty() || n < 1 || n > HW) throw Fail{-EINVAL, "terrain: bad run length"};
            for (int i = 0; i < n - 1; i++) terr.push_back(terr.back());
        }
    } else {
        for (char ch : ts)
            if (!isspace((unsigned char)ch)) terr.push_back(ch - '0');
    }
    if ((int)terr.size() < HW) throw Fail{-EINVAL, "terrain too short"};
    return terr;
}

MapDef parseMap(const std::string& path, const UttInfo& utt) {
    std::ifstream f(path);
    if (!f) throw Fail{-ENOENT, "cannot open map " + path};
    std::stringstream ss;
    ss << f.rdbuf();
    return parseMapText(ss.str(), path, utt);
}

MapDef parseMapText(const std::string& x, const std::string& path, const UttInfo& utt) {
    MapDef m;
    size_t p = x.find("<rts.PhysicalGameState");
    if (p == std::string::npos) throw Fail{-EINVAL, "map: no rts.PhysicalGameState in " + path};
    size_t e = x.find('>', p);
    const std::string root = x.substr(p, e - p);
    m.W = toInt(attrOf(root, "width"));
    m.H = toInt(attrOf(root, "height"));
    if (m.W <= 0 || m.H <= 0 || m.W > 250 || m.H > 250) throw Fail{-EINVAL, "map: unsupported size"};
    const size_t t0 = x.find("<terrain>", e), t1 = x.find("</terrain>", t0);
    if (t0 == std::string::npos || t1 == std::string::npos) throw Fail{-EINVAL, "map: no terrain"};
    const std::string ts = x.substr(t0 + 9, t1 - t0 - 9);
    const int HW = m.W * m.H;
    const std::vector<int> terr = decodeTerrain(ts, HW);
    m.terrain.resize((size_t)HW);
    for (int i = 0; i < HW; i++) m.terrain[(size_t)i] = terr[(size_t)i] != 0;
    const size_t end = x.find("</rts.PhysicalGameState>", t1);
    size_t q = t1;
    int np = 0;
    while (true) {
        const size_t a = x.find("<rts.Player", q);
        if (a == std::string::npos || a > end) break;
        const size_t b = x.find('>', a);
        const std::string pt = x.substr(a, b - a);
        const int id = toInt(attrOf(pt, "ID"));
        if (id != np || np >= 2) throw Fail{-EINVAL, "map: players must be 0 and 1 in order"};
        m.res[np++] = toInt(attrOf(pt, "resources"));
        q = b;
    }
    if (np != 2) throw Fail{-EINVAL, "map: need exactly 2 players"};
    q = t1;
    std::vector<long long> ids;
    std::vector<uint8_t> occ((size_t)HW, 0);
    while (true) {
        const size_t a = x.find("<rts.units.Unit ", q);
        if (a == std::string::npos || a > end) break;
        const size_t b = x.find('>', a);
        const std::string ut = x.substr(a, b - a);
        MapDef::U u;
        const std::string tn = attrOf(ut, "type");
        u.type = utt.typeOf(tn);  // utt.getUnitType(name) (Unit.java:610)
        if (u.type < 0) throw Fail{-EINVAL, "map: unknown unit type " + tn};
        try {
            u.id = std::stoll(attrOf(ut, "ID"));
        } catch (const std::logic_error& e) {  // (no digits, or out of range: the code and text mrts_create gave it)
            throw Fail{-EINVAL, e.what()};
        }
        u.player = toInt(attrOf(ut, "player"));
        u.x = toInt(attrOf(ut, "x"));
        u.y = toInt(attrOf(ut, "y"));
        u.res = toInt(attrOf(ut, "resources"));
        u.hp = toInt(attrOf(ut, "hitpoints"));
        if (u.player < -1 || u.player > 1) throw Fail{-EINVAL, "map: unit player out of range"};
        if (u.x < 0 || u.y < 0 || u.x >= m.W || u.y >= m.H) throw Fail{-EINVAL, "map: unit off the map"};
        if (u.res < -32768 || u.res > 32767 || u.hp < -32768 || u.hp > 32767) throw Fail{-EINVAL, "map: value exceeds int16"};
        if (std::find(ids.begin(), ids.end(), u.id) != ids.end()) throw Fail{-EINVAL, "map: repeated unit ID"};
        if (occ[(size_t)(u.y * m.W + u.x)]) throw Fail{-EINVAL, "map: two units in one position"};  // addUnit :192
        occ[(size_t)(u.y * m.W + u.x)] = 1;
        ids.push_back(u.id);
        m.units.push_back(u);
        q = b;
    }
    return m;
}

// ------------------------------------------------------------------ state blocks
// GameState.toJSON(w, true, false) (rts/GameState.java:819-837) with PhysicalGameState.toJSON
// (:658-691), Player.toJSON (Player.java:86-88), Unit.toJSON (Unit.java:577-588) and
// UnitAction.toJSON (UnitAction.java:569-582).  Unit IDs are list positions: Java's IDs come from a
// JVM-global counter and are not part of a game's reproducible state.
std::string gameToJson(const StateShape& env, const std::vector<int32_t>& s) {
    const int CAP = env.CAP, HW = env.HW;
    const int32_t* A = s.data() + H_WORDS;
    const uint8_t* terr = (const uint8_t*)(s.data() + stateTerrOff(CAP, HW));
    const int nu = s[H_NU];
    std::ostringstream w;
    w << "{\"time\":" << s[H_TIME] << ",\"pgs\":{\"width\":" << env.W << ",\"height\":" << env.H << ",\"terrain\":\"";
    for (int i = 0; i < HW; i++) w << (int)terr[i];
    w << "\",\"players\":[{\"ID\":0, \"resources\":" << s[H_RES0] << "},{\"ID\":1, \"resources\":" << s[H_RES1]
      << "}],\"units\":[";
    struct Asg { int seq, unit; };
    std::vector<Asg> asg;
    for (int i = 0; i < nu; i++) {
        const uint32_t c = (uint32_t)A[A_UC * CAP + i];
        if (i) w << ",";
        w << "{\"type\":\"" << env.uttInfo.names[(c >> 16) & 0xF] << "\", \"ID\":" << i << ", \"player\":"
          << (int)((c >> 20) & 3) - 1 << ", \"x\":" << (c & 0xFF) << ", \"y\":" << ((c >> 8) & 0xFF)
          << ", \"resources\":" << A[A_RES * CAP + i] << ", \"hitpoints\":" << A[A_HP * CAP + i] << "}";
        if ((uint32_t)A[A_UA * CAP + i] & UA_PRESENT) asg.push_back({A[A_AS * CAP + i], i});
    }
    w << "]},\"actions\":[";
    std::sort(asg.begin(), asg.end(), [](const Asg& a, const Asg& b) { return a.seq < b.seq; });
    for (size_t k = 0; k < asg.size(); k++) {
        const int i = asg[k].unit;
        const uint32_t a = (uint32_t)A[A_UA * CAP + i];
        const int t = (int)(a & 0xF), prm = (int16_t)A[A_PAR * CAP + i];
        if (k) w << ",";
        w << "{\"ID\":" << i << ", \"time\":" << A[A_AT * CAP + i] << ", \"action\":{\"type\":" << t;
        if (t == 5) {
            w << ", \"x\":" << ((a >> 8) & 0xFF) << ",\"y\":" << ((a >> 16) & 0xFF);
        } else {
            if (prm != -1) w << ", \"parameter\":" << prm;
            if (t == 4) w << ", \"unitType\":\"" << env.uttInfo.names[(a >> 4) & 0xF] << "\"";
        }
        w << "}}";
    }
    w << "]}";
    return w.str();
}

// GameState.fromJSON (rts/GameState.java:897-915): PhysicalGameState.fromJSON (:735-756, terrain raw
// or A/B), Player.fromJSON, Unit.fromJSON (Unit.java:629-642: hitpoints default 1), the actions by
// unit ID in array order (UnitAction.fromJSON, UnitAction.java:647-658).  A new GameState: time from
// the JSON, unitCancelationCounter 0.  Writes the words of block `s` it describes; everything else
// (random streams, kind, mask row sets) is kept.  Rejects what Java would throw on (unknown type or
// ID, two units in a cell) and what this build cannot hold.
void jsonToBlock(const StateShape& env, const std::string& text, std::vector<int32_t>& s) {
    mjson::Value o;
    try {
        o = mjson::parse(text);
    } catch (const std::runtime_error& e) {
        throw Fail{-EINVAL, std::string("state json: ") + e.what()};
    }
    try {
        const int CAP = env.CAP, HW = env.HW, W = env.W, H = env.H;
        const mjson::Value& pg = o.at("pgs");
        if (pg.getInt("width", 8) != W || pg.getInt("height", 8) != H) throw Fail{-EINVAL, "state json: map size differs from the handle's"};
        const std::vector<int> terr = decodeTerrain(pg.getString("terrain", ""), HW);
        const mjson::Value& pl = pg.at("players");
        if (pl.arr.size() != 2 || pl.arr[0].getInt("ID", -1) != 0 || pl.arr[1].getInt("ID", -1) != 1)
            throw Fail{-ENOTSUP, "state json: players must be 0 and 1"};
        const mjson::Value& us = pg.at("units");
        const int nu = (int)us.arr.size();
        if (nu > env.maxUnits) throw Fail{-ENOSPC, "state json: more units than the handle's max_units"};
        int32_t* A = s.data() + H_WORDS;
        std::vector<int64_t> ids((size_t)nu);
        std::vector<char> occ((size_t)HW, 0);
        for (int a = 0; a < N_ARRAYS; a++)
            for (int i = 0; i < CAP; i++) A[a * CAP + i] = 0;
        for (int i = 0; i < nu; i++) {
            const mjson::Value& u = us.arr[(size_t)i];
            const int type = env.uttInfo.typeOf(u.getString("type", ""));
            const int p = u.getInt("player", -1), x = u.getInt("x", 0), y = u.getInt("y", 0);
            const int r = u.getInt("resources", 0), hp = u.getInt("hitpoints", 1);
            ids[(size_t)i] = u.getLong("ID", -1);
            if (type < 0) throw Fail{-EINVAL, "state json: unknown unit type"};
            if (p < -1 || p > 1 || x < 0 || y < 0 || x >= W || y >= H) throw Fail{-EINVAL, "state json: unit out of range"};
            if (r < -32768 || r > 32767 || hp < -32768 || hp > 32767) throw Fail{-EINVAL, "state json: value exceeds int16"};
            if (occ[(size_t)(y * W + x)]) throw Fail{-EINVAL, "state json: two units in one position (addUnit)"};
            for (int j = 0; j < i; j++)
                if (ids[(size_t)j] == ids[(size_t)i]) throw Fail{-EINVAL, "state json: repeated unit ID"};
            occ[(size_t)(y * W + x)] = 1;
            A[A_UC * CAP + i] = (int32_t)((uint32_t)x | ((uint32_t)y << 8) | ((uint32_t)type << 16) | ((uint32_t)(p + 1) << 20));
            A[A_HP * CAP + i] = hp;
            A[A_RES * CAP + i] = r;
            A[A_PAR * CAP + i] = -1;
        }
        const mjson::Value& acts = o.at("actions");
        int seq = 0;
        for (auto& av : acts.arr) {
            const int64_t id = av.getLong("ID", -1);
            int i = 0;
            while (i < nu && ids[(size_t)i] != id) i++;
            if (i == nu) throw Fail{-EINVAL, "state json: action for an unknown unit ID"};
            const uint32_t c = (uint32_t)A[A_UC * CAP + i];
            if ((int)((c >> 20) & 3) - 1 < 0) throw Fail{-EINVAL, "state json: action for a neutral unit"};
            const mjson::Value& ua = av.at("action");
            const int t = ua.getInt("type", 0), prm = ua.getInt("parameter", -1);
            const int tx = ua.getInt("x", -1), ty = ua.getInt("y", -1);
            const std::string utn = ua.getString("unitType", "");
            int ut = 0;
            if (t < 0 || t > 5) throw Fail{-EINVAL, "state json: bad action type"};
            if (t == 5 && (tx < 0 || ty < 0 || tx >= W || ty >= H)) throw Fail{-ENOTSUP, "state json: attack target off the map"};
            if (t >= 1 && t <= 4 && (prm < 0 || prm > 3)) throw Fail{-ENOTSUP, "state json: bad direction"};
            if (t == 1 || t == 4) {  // UnitAction.execute writes the target cell unguarded (HARVEST / RETURN test it first)
                static const int DX[4] = {0, 1, 0, -1}, DY[4] = {-1, 0, 1, 0};  // UP, RIGHT, DOWN, LEFT
                const int nx = (int)(c & 0xFF) + DX[prm], ny = (int)((c >> 8) & 0xFF) + DY[prm];
                if (nx < 0 || ny < 0 || nx >= W || ny >= H)
                    throw Fail{-ENOTSUP, t == 1 ? "state json: move target off the map" : "state json: produce target off the map"};
            }
            if (t == 0 && (prm < -1 || prm > 32767)) throw Fail{-ENOTSUP, "state json: bad NONE duration"};
            if (t == 4) {
                ut = env.uttInfo.typeOf(utn);
                if (ut < 0) throw Fail{-EINVAL, "state json: unknown produced type"};
            }
            const bool again = (uint32_t)A[A_UA * CAP + i] & UA_PRESENT;  // put() on a present key keeps its place
            A[A_UA * CAP + i] = (int32_t)((uint32_t)t | ((uint32_t)ut << 4) |
                                          (t == 5 ? ((uint32_t)tx << 8) | ((uint32_t)ty << 16) : 0u) | UA_PRESENT);
            A[A_PAR * CAP + i] = t == 5 ? -1 : prm;
            A[A_AT * CAP + i] = av.getInt("time", 0);
            if (!again) A[A_AS * CAP + i] = seq++;
        }
        const mjson::Value& p0 = pl.arr[0];
        const mjson::Value& p1 = pl.arr[1];
        s[H_TIME] = o.getInt("time", 0);
        s[H_NU] = nu;
        s[H_RES0] = p0.getInt("resources", 0);
        s[H_RES1] = p1.getInt("resources", 0);
        s[H_SEQ] = seq;
        s[H_STEPS] = 0;
        s[H_ERR] = 0;
        s[H_CANCEL_CNT] = 0;
        uint8_t* tb = (uint8_t*)(s.data() + stateTerrOff(CAP, HW));
        for (int i = 0; i < HW; i++) tb[i] = terr[(size_t)i] != 0;
        for (int i = HW; i < 4 * ((HW + 3) / 4); i++) tb[i] = 0;
        for (int i = 0; i < nu; i++) {  // units may not stand on walls (the cell map has one owner per cell)
            const uint32_t c = (uint32_t)A[A_UC * CAP + i];
            if (tb[(c & 0xFF) + ((c >> 8) & 0xFF) * W]) throw Fail{-ENOTSUP, "state json: unit on a wall"};
        }
    } catch (const std::runtime_error& e) {
        throw Fail{-EINVAL, std::string("state json: ") + e.what()};
    }
}

std::vector<int32_t> canonicalDump(const int32_t* s, int CAP) {
    const int32_t* A = s + H_WORDS;
    const int nu = s[H_NU];
    std::vector<int32_t> d;
    d.push_back(s[H_TIME]);
    d.push_back(2);
    d.push_back(s[H_RES0]);
    d.push_back(s[H_RES1]);
    d.push_back(nu);
    struct Asg { int seq, unit; };
    std::vector<Asg> asg;
    for (int i = 0; i < nu; i++) {
        const uint32_t c = (uint32_t)A[A_UC * CAP + i];
        d.push_back((int32_t)((c >> 16) & 0xF));
        d.push_back((int32_t)((c >> 20) & 3) - 1);
        d.push_back((int32_t)(c & 0xFF));
        d.push_back((int32_t)((c >> 8) & 0xFF));
        d.push_back(A[A_HP * CAP + i]);
        d.push_back(A[A_RES * CAP + i]);
        if ((uint32_t)A[A_UA * CAP + i] & UA_PRESENT) asg.push_back({A[A_AS * CAP + i], i});
    }
    std::sort(asg.begin(), asg.end(), [](const Asg& a, const Asg& b) { return a.seq < b.seq; });
    d.push_back((int32_t)asg.size());
    for (auto& e : asg) {
        const uint32_t a = (uint32_t)A[A_UA * CAP + e.unit];
        const int t = (int)(a & 0xF);
        d.push_back(e.unit);
        d.push_back(t);
        d.push_back(t == 5 ? -1 : A[A_PAR * CAP + e.unit]);
        d.push_back(t == 5 ? (int32_t)((a >> 8) & 0xFF) : 0);
        d.push_back(t == 5 ? (int32_t)((a >> 16) & 0xFF) : 0);
        d.push_back(t == 4 ? (int32_t)((a >> 4) & 0xF) : -1);
        d.push_back(A[A_AT * CAP + e.unit]);
    }
    return d;
}

bool valuesFitBytes(const int32_t* s, int CAP) {
    const int nu = s[H_NU];
    const int32_t* A = s + H_WORDS;
    for (int i = 0; i < nu && i < CAP; i++) {
        const int hpv = A[A_HP * CAP + i], rv = A[A_RES * CAP + i];
        if (hpv < 0 || hpv > 255 || rv < 0 || rv > 255) return false;
    }
    return true;
}

// ------------------------------------------------------------------ a handle's configuration
CreatePlan planCreate(const mrts_config* cfg) {
    if (cfg->n_selfplay_slots < 0 || (cfg->n_selfplay_slots & 1)) throw Fail{-EINVAL, "n_selfplay_slots must be even"};
    if (cfg->n_bot_envs < 0) throw Fail{-EINVAL, "n_bot_envs < 0"};
    const int nSlots = cfg->n_selfplay_slots + cfg->n_bot_envs;
    if (nSlots <= 0) throw Fail{-EINVAL, "no environments"};
    if (!cfg->map_paths) throw Fail{-EINVAL, "map_paths is null"};
    CreatePlan P;
    HandleConfig* const env = &P.cfg;
    env->device = cfg->device;
    env->uttInfo = cfg->utt_json ? uttFromJson(cfg->utt_json) : makeUtt(cfg->utt_version, cfg->conflict_policy);
    env->utt = env->uttInfo.dev;
    env->K = env->utt.K;
    env->C = cfg->partial_obs ? 8 : 6;
    env->partialObs = cfg->partial_obs;
    env->maxSteps = cfg->max_steps;
    env->nSlots = nSlots;
    env->nSpGames = cfg->n_selfplay_slots / 2;
    env->nGames = env->nSpGames + cfg->n_bot_envs;
    env->slotIdBase = (uint32_t)cfg->slot_id_base;
    env->maskDelta = cfg->mask_delta;
    if (cfg->n_rewards < 0 || cfg->n_rewards > MAX_REWARDS) throw Fail{-EINVAL, "n_rewards must be 0..8"};
    if (cfg->n_rewards > 0) {
        if (!cfg->reward_kinds) throw Fail{-EINVAL, "reward_kinds is null"};
        env->rewardKinds.assign(cfg->reward_kinds, cfg->reward_kinds + cfg->n_rewards);
        for (int k : env->rewardKinds)
            if (k < 0 || k >= RF_COUNT) throw Fail{-EINVAL, "unknown reward function"};
    }
    if (cfg->ai1_kinds && cfg->n_selfplay_slots) throw Fail{-EINVAL, "the bot-only client has no self-play slots"};
    env->forwardModel = cfg->forward_model ? 1 : 0;
    env->botOnly = cfg->ai1_kinds ? 1 : 0;
    if (env->forwardModel && !cfg->ai1_kinds) throw Fail{-EINVAL, "a forward model needs ai1_kinds (player 0's playout policy)"};
    if (env->forwardModel && cfg->partial_obs) throw Fail{-EINVAL, "a forward model plays on the full state (partial_obs must be 0)"};
    env->gameKindHost.assign((size_t)env->nGames, 0);  // self-play = 0
    for (int j = 0; j < cfg->n_bot_envs; j++) {
        const int k2 = cfg->bot_kinds ? cfg->bot_kinds[j] : MRTS_BOT_PASSIVE;
        const int k1 = cfg->ai1_kinds ? cfg->ai1_kinds[j] : MRTS_BOT_PASSIVE;
        if (k1 < 0 || k1 > MRTS_BOT_LIGHT_RUSH || k2 < 0 || k2 > MRTS_BOT_LIGHT_RUSH)
            throw Fail{-ENOTSUP, "only PassiveAI / RandomBiasedAI / LightRush are native"};
        const int type = env->forwardModel ? 3 : (cfg->ai1_kinds ? 2 : 1);  // GT_PLAYOUT / BOT_VS_BOT / AGENT_VS_BOT
        if (k1 == MRTS_BOT_LIGHT_RUSH || k2 == MRTS_BOT_LIGHT_RUSH) {
            // refused, not approximated: a playout policy has no memory to carry between copies of a game, and
            // JNIGridnetClient.gameStep runs the opponent on its PartiallyObservableGameState
            // (tests/JNIGridnetClient.java:164-173) — LightRush on a view is a different bot
            if (env->forwardModel)
                throw Fail{-ENOTSUP, "LightRush is not available as a forward-model playout policy (its memory of abstract "
                                     "actions is not part of a copied game)"};
            if (cfg->partial_obs && type == 1)
                throw Fail{-ENOTSUP, "partial_obs + LightRush opponent: Java runs the bot on the player's partially "
                                     "observable view, which this build does not compute for LightRush"};
            int ids[4] = {-1, -1, -1, -1};
            static const char* const need[4] = {"Base", "Barracks", "Worker", "Light"};
            for (int q = 0; q < 4; q++)
                for (int t = 0; t < env->utt.ntypes; t++)
                    if (env->uttInfo.names[(size_t)t] == need[q] && ids[q] < 0) ids[q] = t;
            for (int q = 0; q < 4; q++)
                if (ids[q] < 0)
                    throw Fail{-ENOTSUP, std::string("LightRush needs a unit type named ") + need[q] + " in the unit-type table"};
            env->botTypes = (uint32_t)ids[0] | ((uint32_t)ids[1] << 4) | ((uint32_t)ids[2] << 8) | ((uint32_t)ids[3] << 12);
            env->hasLightRush = 1;
        }
        env->gameKindHost[(size_t)(env->nSpGames + j)] = type | (k1 << 4) | (k2 << 8);
        // JNIGridnetClient.gameStep runs the opponent on its PartiallyObservableGameState
        // (tests/JNIGridnetClient.java:164-173).  The GPU RandomBiasedAI takes getUnitActions of an
        // owned unit from the full cell map, which equals the view's only when every cell the unit
        // can act on (its 4 neighbours, its attack disk) lies inside its own sight disk.  Every
        // built-in table satisfies that; a custom table that does not is refused, not run with
        // different action lists.
        if (cfg->partial_obs && type == 1 && k2 == MRTS_BOT_RANDOM_BIASED) {
            const DevUtt& u = env->utt;
            for (int t = 0; t < u.ntypes; t++) {
                const bool acts = (u.flags[t] & (F_MOVE | F_ATTACK | F_HARVEST)) || u.nprod[t] > 0;
                const int need = std::max(1, (u.flags[t] & F_ATTACK) ? u.range[t] : 1);
                if (acts && u.sight[t] < need)
                    throw Fail{-ENOTSUP, "partial_obs + RandomBiasedAI: unit type " + env->uttInfo.names[(size_t)t] +
                                             " has sightRadius < max(1, attackRange); its PO action list would "
                                             "differ from the full-state one this build computes"};
            }
        }
    }
    // maps: one template per distinct path
    std::map<std::string, int> tmplIndex;
    std::vector<MapDef> maps;
    std::vector<int> gameTmpl((size_t)env->nGames);
    for (int g = 0; g < env->nGames; g++) {
        const int slot = g < env->nSpGames ? 2 * g : 2 * env->nSpGames + (g - env->nSpGames);
        const char* p = cfg->map_paths[slot];
        if (!p) throw Fail{-EINVAL, "null map path"};
        auto it = tmplIndex.find(p);
        if (it == tmplIndex.end()) {
            maps.push_back(parseMap(p, env->uttInfo));
            it = tmplIndex.emplace(p, (int)maps.size() - 1).first;
        }
        gameTmpl[(size_t)g] = it->second;
    }
    env->H = maps[0].H;
    env->W = maps[0].W;
    env->HW = env->H * env->W;
    for (auto& m : maps)
        if (m.H != env->H || m.W != env->W) throw Fail{-EINVAL, "all maps must share env 0's size (JNIGridnetVecClient.java:127-133)"};
    // capacity: one live unit per cell, plus slack for the step's births over its deaths
    // unit slots: at most one live unit per cell, plus slack for the births of a step over its
    // deaths (dead slots are compacted at the end of the step).  max_units lowers the bound on
    // live units (fewer LDS bytes per game -> more games resident per CU); a game that would
    // exceed it sets MRTS_ERR_CAPACITY instead of continuing.
    if (cfg->max_units < 0) throw Fail{-EINVAL, "max_units < 0"};
    const int maxUnits = cfg->max_units ? std::min(cfg->max_units, env->HW) : env->HW;
    env->CAP = maxUnits + std::max(64, maxUnits / 4);
    env->maxUnits = maxUnits;
    if (env->CAP > 0xFFF0) throw Fail{-EINVAL, "map too large"};
    if ((size_t)env->nSlots * env->HW >= (size_t)1 << 31) throw Fail{-EINVAL, "n_slots * H * W must be < 2^31"};
    if (env->hasLightRush && env->HW > LR_MAX_CELLS)
        throw Fail{-ENOTSUP, "LightRush: the map has more than 1024 cells (the size limit of the native A* pathfinder)"};
    // everything above is validation (mrts_create's device work starts after it); nothing below can refuse
    for (auto& m : maps) P.mostMapUnits = std::max(P.mostMapUnits, (int)m.units.size());
    {  // the hp / resources range an observation plane can show: the maps' units, the table's types
        // (a unit's hp only falls; its resources fall, or rise by harvestAmount from 0).  A state
        // injected later (mrts_set_state_json, mrts_restore) can hold other values: noteValues.
        int mx = 0, mn = 0;
        for (auto& m : maps)
            for (auto& u : m.units) {
                mx = std::max(mx, std::max(u.hp, u.res));
                mn = std::min(mn, std::min(u.hp, u.res));
            }
        for (int t = 0; t < env->utt.ntypes; t++) mx = std::max(mx, std::max(env->utt.hp[t], env->utt.harvestAmt[t]));
        env->obsImg = (mx <= 255 && mn >= 0) ? 1 : 0;
    }
    // templates blob
    std::vector<int32_t>& blob = P.blob;
    std::vector<int> off;
    for (auto& m : maps) {
        off.push_back((int)blob.size());
        const int nu = (int)m.units.size();
        blob.push_back(m.H);
        blob.push_back(m.W);
        blob.push_back(m.res[0]);
        blob.push_back(m.res[1]);
        blob.push_back(nu);
        std::vector<int32_t> terr((size_t)(env->HW + 3) / 4, 0);
        std::memcpy(terr.data(), m.terrain.data(), (size_t)env->HW);
        blob.insert(blob.end(), terr.begin(), terr.end());
        for (auto& u : m.units)
            blob.push_back((int32_t)((uint32_t)u.x | ((uint32_t)u.y << 8) | ((uint32_t)u.type << 16) | ((uint32_t)(u.player + 1) << 20)));
        for (auto& u : m.units) blob.push_back(u.hp);
        for (auto& u : m.units) blob.push_back(u.res);
    }
    env->tmplOffHost.resize((size_t)env->nGames);
    for (int g = 0; g < env->nGames; g++) env->tmplOffHost[(size_t)g] = off[(size_t)gameTmpl[(size_t)g]];
    {  // what a state block does not carry but its meaning depends on: a restore must match it
        uint32_t hv = 2166136261u;
        auto mix = [&hv](const void* p, size_t n) {
            for (size_t i = 0; i < n; i++) hv = (hv ^ ((const uint8_t*)p)[i]) * 16777619u;
        };
        mix(env->gameKindHost.data(), env->gameKindHost.size() * 4);
        mix(blob.data(), blob.size() * 4);
        mix(env->tmplOffHost.data(), env->tmplOffHost.size() * 4);
        mix(&env->maxSteps, 4);
        mix(&env->partialObs, sizeof(env->partialObs));
        const int nrk = (int)env->rewardKinds.size();
        mix(&nrk, 4);
        mix(env->rewardKinds.data(), env->rewardKinds.size() * sizeof(env->rewardKinds[0]));
        env->cfgHash = hv;
    }
    // headers: java.util.Random seeds per game (same derivation as the CPU oracle)
    P.rngWords.assign((size_t)6 * env->nGames, 0);
    auto scramble = [](uint64_t s) { return (s ^ 0x5DEECE66DULL) & ((1ULL << 48) - 1); };
    for (int g = 0; g < env->nGames; g++) {
        const int slot = g < env->nSpGames ? 2 * g : 2 * env->nSpGames + (g - env->nSpGames);
        const uint64_t es = cfg->seed + (uint64_t)(env->slotIdBase + (uint32_t)slot);
        int32_t* h = &P.rngWords[(size_t)6 * g];  // h[w - H_RNG_CANCEL] = header word w
        const uint64_t rc = scramble(es ^ 0x9E3779B97F4A7C15ULL), rd = scramble(es ^ 0xC2B2AE3D27D4EB4FULL), rs = scramble(es);
        h[0] = (int32_t)(uint32_t)rc;
        h[1] = (int32_t)(uint32_t)(rc >> 32);
        h[H_RNG_DAMAGE - H_RNG_CANCEL] = (int32_t)(uint32_t)rd;
        h[H_RNG_DAMAGE - H_RNG_CANCEL + 1] = (int32_t)(uint32_t)(rd >> 32);
        h[H_RNG_SAMPLER - H_RNG_CANCEL] = (int32_t)(uint32_t)rs;
        h[H_RNG_SAMPLER - H_RNG_CANCEL + 1] = (int32_t)(uint32_t)(rs >> 32);
    }
    return P;
}

// ------------------------------------------------------------------ whole-handle checkpoint
CkptHeader ckptHeader(const HandleConfig& c) {
    CkptHeader h;
    std::memset(&h, 0, sizeof(h));
    std::memcpy(h.magic, "MRTSCKP1", 8);
    h.version = 3;
    h.H = c.H;
    h.W = c.W;
    h.CAP = c.CAP;
    h.nGames = c.nGames;
    h.nSpGames = c.nSpGames;
    h.words = (int32_t)c.blockWords();
    h.uttHash = uttHash(c.utt);
    h.cfgHash = c.cfgHash;
    return h;
}

void checkCkpt(const HandleConfig& c, const void* buf, int64_t size) {
    CkptHeader h;
    if (size < (int64_t)sizeof(h)) throw Fail{-EINVAL, "checkpoint too short"};
    std::memcpy(&h, buf, sizeof(h));
    if (std::memcmp(h.magic, "MRTSCKP1", 8) != 0 || h.version != 3) throw Fail{-EINVAL, "not a checkpoint"};
    const CkptHeader w = ckptHeader(c);
    if (h.H != w.H || h.W != w.W || h.CAP != w.CAP || h.nGames != w.nGames || h.nSpGames != w.nSpGames || h.words != w.words ||
        h.uttHash != w.uttHash)
        throw Fail{-EINVAL, "checkpoint of a different configuration"};
    if (h.cfgHash != w.cfgHash)
        throw Fail{-EINVAL, "checkpoint of a different configuration (opponents, maps, max_steps, reward functions "
                            "or partial observability differ)"};
    if (size != ckptSize(c)) throw Fail{-EINVAL, "checkpoint size mismatch"};
}

// ------------------------------------------------------------------ packed observation rows
ObsPackParams obsPackShape(const HandleConfig& c, int32_t n_rows, int32_t cap) {
    if (c.HW > OBS_MAX_CELLS || (c.C != 6 && c.C != 8))
        throw Fail{-ENOTSUP, "packed observation rows: maps of at most 65536 cells, 6 or 8 planes"};
    if (n_rows < 0 || (int64_t)n_rows * c.HW >= ((int64_t)1 << 31)) throw Fail{-EINVAL, "n_rows: 0 <= n_rows * H*W < 2^31"};
    if (cap < 1 || cap > c.HW) throw Fail{-EINVAL, "cap: 1 <= cap <= H*W"};
    ObsPackParams P;
    std::memset(&P, 0, sizeof(P));
    P.HW = c.HW;
    P.C = c.C;
    P.cap = cap;
    P.words = obsPackedWords(c.C, c.HW, cap);
    P.n_rows = n_rows;
    return P;
}
void obsPackBuffers(ObsPackParams& P, const int32_t* d_obs, uint32_t* d_out) {
    if (!d_obs || !d_out) throw Fail{-EINVAL, "null argument"};
    if (((uintptr_t)d_obs & 3) || ((uintptr_t)d_out & 3)) throw Fail{-EINVAL, "misaligned buffer"};
    P.obs = d_obs;
    P.packed_out = d_out;
}
void obsPackedSource(ObsPackParams& P, const uint32_t* d_packed, int32_t n_packed, const int32_t* d_index, const void* d_out,
                     int out_align) {
    if (!d_packed || !d_out) throw Fail{-EINVAL, "null argument"};
    if (n_packed < 1 || (!d_index && n_packed < P.n_rows)) throw Fail{-EINVAL, "n_packed: at least 1, and n_rows without an index"};
    if (((uintptr_t)d_packed & 3) || ((uintptr_t)d_index & 3) || ((uintptr_t)d_out & (uintptr_t)(out_align - 1)))
        throw Fail{-EINVAL, "misaligned buffer"};
    P.packed = d_packed;
    P.n_packed = n_packed;
    P.index = d_index;
}

}  // namespace mrts

// ------------------------------------------------------------------ internal probes
// The state converters without a handle, for the CPU tests (tests/test_state_json_cpu.py; not in include/mrts.h):
// state_json goes into a zeroed block of a handle of this shape through jsonToBlock, and the block comes back as
// gameToJson's text (mrts_internal_state_probe) or as the canonical dump's words (mrts_internal_dump_probe).  Both
// return the characters / words written to out, or the refusal's code with its text in err.
namespace {
template <class T, class Read>
int stateProbe(int H, int W, int CAP, int max_units, int utt_version, int conflict_policy, const char* utt_json,
               const char* state_json, T* out, int cap, char* err, int err_cap, Read read) {
    std::string msg;
    const int r = mrts::guardCall(msg, [&] {
        if (!state_json || !out || H < 1 || W < 1 || H > 250 || W > 250 || max_units < 0 || max_units > CAP)
            throw mrts::Fail{-EINVAL, "bad argument"};
        mrts::StateShape sh;
        sh.H = H, sh.W = W, sh.HW = H * W, sh.CAP = CAP, sh.maxUnits = max_units;
        sh.uttInfo = utt_json ? mrts::uttFromJson(utt_json) : mrts::makeUtt(utt_version, conflict_policy);
        std::vector<int32_t> s((size_t)mrts::stateWords(CAP, sh.HW), 0);
        mrts::jsonToBlock(sh, state_json, s);
        const auto v = read(sh, s);
        if (v.size() > (size_t)cap) throw mrts::Fail{-ENOSPC, "buffer too small"};
        std::copy(v.begin(), v.end(), out);
        return (int)v.size();
    });
    if (err && err_cap > 0) std::snprintf(err, (size_t)err_cap, "%s", r < 0 ? msg.c_str() : "");
    return r;
}
}  // namespace

extern "C" int mrts_internal_state_probe(int H, int W, int CAP, int max_units, int utt_version, int conflict_policy,
                                         const char* utt_json, const char* state_json, char* out, int cap, char* err,
                                         int err_cap) {
    return stateProbe(H, W, CAP, max_units, utt_version, conflict_policy, utt_json, state_json, out, cap, err, err_cap,
                      [](const mrts::StateShape& sh, const std::vector<int32_t>& s) { return mrts::gameToJson(sh, s); });
}

extern "C" int mrts_internal_dump_probe(int H, int W, int CAP, int max_units, int utt_version, int conflict_policy,
                                        const char* utt_json, const char* state_json, int32_t* out, int cap, char* err,
                                        int err_cap) {
    return stateProbe(H, W, CAP, max_units, utt_version, conflict_policy, utt_json, state_json, out, cap, err, err_cap,
                      [](const mrts::StateShape& sh, const std::vector<int32_t>& s) { return mrts::canonicalDump(s.data(), sh.CAP); });
}
