// hostcheck.cpp — `make hostcheck`: mrts_hostdata.cpp on its own under the address and undefined-behaviour
// sanitizers (a CPU program; nothing of it is in libmrts.so).  usage: hostcheck <utt.json> <map.xml>...
//   * every map parses under the original table, and one state per map size (the map's own units, with a MOVE, an
//     ATTACK_LOCATION and a PRODUCE under way) round-trips: text -> block -> the same text, and its dump -> the
//     same dump after a second trip;
//   * the three built-in tables under each conflict policy, and the table file, round-trip through JSON;
//   * every proper prefix of the smallest map, of the table file and of the smallest map's state goes to its parser:
//     each must end in a Fail or a clean parse;
//   * a MOVE or PRODUCE under way that points off the map is refused, from each of the four edges; a HARVEST or
//     RETURN that does, and any of them along the edge, is kept;
//   * the packed observation rows' word count and every refusal of their argument checks.
// Any other exception leaves main (std::terminate), a sanitizer report aborts: both fail the make target.
#include <cstdio>
#include <fstream>
#include <set>
#include <sstream>

#include "mrts_hostdata.h"

using namespace mrts;

static std::string slurp(const std::string& path) {
    std::ifstream f(path);
    if (!f) throw Fail{-ENOENT, "cannot open " + path};
    std::stringstream ss;
    ss << f.rdbuf();
    return ss.str();
}

static int g_bad = 0;
static void expect(bool ok, const std::string& what) {
    if (ok) return;
    std::printf("FAILED: %s\n", what.c_str());
    g_bad++;
}

// the map's initial state as GameState.toJSON writes it (unit IDs = list positions), with up to three actions
static std::string stateOf(const MapDef& m, const UttInfo& utt) {
    std::ostringstream w;
    w << "{\"time\":7,\"pgs\":{\"width\":" << m.W << ",\"height\":" << m.H << ",\"terrain\":\"";
    for (uint8_t t : m.terrain) w << (int)t;
    w << "\",\"players\":[{\"ID\":0, \"resources\":" << m.res[0] << "},{\"ID\":1, \"resources\":" << m.res[1] << "}],\"units\":[";
    std::vector<std::string> acts;
    for (size_t i = 0; i < m.units.size(); i++) {
        const MapDef::U& u = m.units[i];
        w << (i ? "," : "") << "{\"type\":\"" << utt.names[(size_t)u.type] << "\", \"ID\":" << i << ", \"player\":" << u.player
          << ", \"x\":" << u.x << ", \"y\":" << u.y << ", \"resources\":" << u.res << ", \"hitpoints\":" << u.hp << "}";
        if (u.player < 0 || acts.size() == 3) continue;
        // (the MOVE goes down and the PRODUCE right, or from the last row / column up and left: a target on the map)
        const std::string kinds[3] = {std::string("{\"type\":1, \"parameter\":") + (u.y + 1 < m.H ? "2}" : "0}"),
                                      "{\"type\":5, \"x\":0,\"y\":0}",
                                      std::string("{\"type\":4, \"parameter\":") + (u.x + 1 < m.W ? "1" : "3") +
                                          ", \"unitType\":\"Worker\"}"};
        acts.push_back("{\"ID\":" + std::to_string(i) + ", \"time\":" + std::to_string(3 + acts.size()) + ", \"action\":" +
                       kinds[acts.size()] + "}");
    }
    w << "]},\"actions\":[";
    for (size_t k = 0; k < acts.size(); k++) w << (k ? "," : "") << acts[k];
    w << "]}";
    return w.str();
}

static StateShape shapeOf(const MapDef& m, const UttInfo& utt) {
    StateShape sh;
    sh.H = m.H, sh.W = m.W, sh.HW = m.H * m.W, sh.maxUnits = sh.HW;
    sh.CAP = sh.maxUnits + std::max(64, sh.maxUnits / 4);
    sh.uttInfo = utt;
    return sh;
}

// runs parse(text[0:n]) for every n < size: a Fail or a clean parse -> (refused, parsed)
template <class F>
static void prefixes(const char* what, const std::string& text, F parse) {
    size_t refused = 0, parsed = 0;
    for (size_t n = 0; n < text.size(); n++) {
        try {
            parse(text.substr(0, n));
            parsed++;
        } catch (const Fail&) {
            refused++;
        }
    }
    std::printf("%s: %zu proper prefixes, %zu refused with an error code, %zu parsed\n", what, text.size(), refused, parsed);
}

int main(int argc, char** argv) {
    std::setvbuf(stdout, nullptr, _IOLBF, 0);  // what ran before an abort stays readable
    if (argc < 3) {
        std::printf("usage: hostcheck <utt.json> <map.xml>...\n");
        return 2;
    }
    const UttInfo utt = makeUtt(1, 1);
    // maps, and one state per map size
    std::set<std::pair<int, int>> sizes;
    std::string smallMap, smallState;
    StateShape smallShape;
    size_t units = 0;
    for (int a = 2; a < argc; a++) {
        const MapDef m = parseMap(argv[a], utt);
        units += m.units.size();
        const std::string text = slurp(argv[a]);
        const bool first = sizes.insert({m.H, m.W}).second;
        if (smallMap.empty() || text.size() < smallMap.size()) {
            smallMap = text;
            smallShape = shapeOf(m, utt);
            smallState = stateOf(m, utt);
        }
        if (!first) continue;
        const StateShape sh = shapeOf(m, utt);
        const std::string j = stateOf(m, utt);
        std::vector<int32_t> s((size_t)stateWords(sh.CAP, sh.HW), 0), s2 = s;
        jsonToBlock(sh, j, s);
        const std::string back = gameToJson(sh, s);
        expect(back == j, std::string("state round trip of ") + argv[a]);
        jsonToBlock(sh, back, s2);
        expect(canonicalDump(s.data(), sh.CAP) == canonicalDump(s2.data(), sh.CAP) && s == s2, std::string("dump round trip of ") + argv[a]);
        expect(valuesFitBytes(s.data(), sh.CAP) == valuesFitBytes(s2.data(), sh.CAP), "valuesFitBytes");
    }
    std::printf("maps: %d parsed, %zu units, %zu sizes; one state per size round-tripped\n", argc - 2, units, sizes.size());
    // unit-type tables
    int tables = 0;
    for (int v = 1; v <= 3; v++)
        for (int crs = 1; crs <= 3; crs++, tables++) {
            const UttInfo B = makeUtt(v, crs);
            const std::string j = uttToJson(B);
            UttInfo I = uttFromJson(j);
            expect(uttToJson(uttFromJson(uttToJson(I))) == uttToJson(I), "built-in table JSON round trip");
            // fromJSON reads harvestTime from "produceTime" (UnitType.java:227): the tables differ there, and only there
            for (int t = 0; t < B.dev.ntypes; t++) I.dev.harvestT[t] = B.dev.harvestT[t];
            expect(uttToJson(I) == j && uttHash(I.dev) == uttHash(B.dev), "built-in table fields");
        }
    const std::string fileUtt = slurp(argv[1]);
    const UttInfo F = uttFromJson(fileUtt);
    expect(uttToJson(uttFromJson(uttToJson(F))) == uttToJson(F), "table file JSON round trip");
    expect(uttHash(F.dev) == uttHash(uttFromJson(fileUtt).dev), "table hash");
    std::printf("unit-type tables: %d built-in and %s round-tripped through JSON\n", tables, argv[1]);
    // truncated inputs
    prefixes("map", smallMap, [&](const std::string& t) { parseMapText(t, "prefix", utt); });
    prefixes("unit-type table", fileUtt, [&](const std::string& t) { uttFromJson(t); });
    prefixes("state", smallState, [&](const std::string& t) {
        std::vector<int32_t> s((size_t)stateWords(smallShape.CAP, smallShape.HW), 0);
        jsonToBlock(smallShape, t, s);
    });
    // an action under way whose target cell lies off the map: MOVE and PRODUCE are refused (UnitAction.execute writes
    // that cell unguarded), HARVEST and RETURN are kept (execute tests the cell first), as is a move along the edge
    {
        StateShape sh;
        sh.H = 3, sh.W = 3, sh.HW = 9, sh.maxUnits = 9, sh.CAP = 9 + 64;
        sh.uttInfo = utt;
        static const int at[4][2] = {{1, 0}, {2, 1}, {1, 2}, {0, 1}};  // a cell on the edge direction d leaves by
        int refused = 0, kept = 0;
        for (int d = 0; d < 4; d++)
            for (int t = 1; t <= 4; t++)
                for (int side = 0; side < 2; side++) {  // off the map, then along the edge
                    const int dir = side ? (d + 1) % 4 : d;
                    std::ostringstream w;
                    w << "{\"time\":9,\"pgs\":{\"width\":3,\"height\":3,\"terrain\":\"000000000\",\"players\":[{\"ID\":0, "
                         "\"resources\":5},{\"ID\":1, \"resources\":5}],\"units\":[{\"type\":\"" << (t == 4 ? "Base" : "Worker")
                      << "\", \"ID\":0, \"player\":0, \"x\":" << at[d][0] << ", \"y\":" << at[d][1]
                      << ", \"resources\":0, \"hitpoints\":1}]},\"actions\":[{\"ID\":0, \"time\":8, \"action\":{\"type\":" << t
                      << ", \"parameter\":" << dir << (t == 4 ? ", \"unitType\":\"Worker\"" : "") << "}}]}";
                    std::vector<int32_t> s((size_t)stateWords(sh.CAP, sh.HW), 0);
                    int rc = 0;
                    try {
                        jsonToBlock(sh, w.str(), s);
                    } catch (const Fail& e) {
                        rc = e.code;
                        expect(e.msg.rfind("state json:", 0) == 0, "off-map refusal's text");
                    }
                    const bool off = !side && (t == 1 || t == 4);
                    expect(rc == (off ? -ENOTSUP : 0), "action type " + std::to_string(t) + " direction " + std::to_string(dir) +
                                                           (side ? " along the edge" : " off the map"));
                    (rc ? refused : kept)++;
                }
        std::printf("actions at the map's edge: %d off-map MOVE / PRODUCE refused, %d others kept\n", refused, kept);
    }
    // packed observation rows: the word count and every refusal of the argument checks (no buffer is dereferenced)
    {
        static_assert(obsPackedWords(6, 256, 128) == 265 && obsPackedWords(8, 1024, 128) == 353 && obsPackedWords(6, 72, 72) == 148,
                      "1 + 2 * cap + (C - 5) * ceil(H*W / 32)");
        HandleConfig c;
        c.H = 9, c.W = 8, c.HW = 72, c.C = 8;
        alignas(16) static uint32_t buf[8];
        const auto code = [](auto&& f) {
            try {
                f();
                return 0;
            } catch (const Fail& e) {
                return e.code;
            }
        };
        int refused = 0, passed = 0;
        const auto want = [&](int rc, auto&& f, const char* what) {
            const int got = code(f);
            expect(got == rc, std::string("packed observation rows: ") + what);
            (got ? refused : passed)++;
        };
        want(0, [&] { expect(obsPackShape(c, 5, 72).words == 1 + 144 + 9, "words of 9x8 x 8 planes"); }, "cap = H*W");
        want(0, [&] { obsPackShape(c, 0, 1); }, "no rows, cap 1");
        want(-EINVAL, [&] { obsPackShape(c, -1, 8); }, "n_rows < 0");
        want(-EINVAL, [&] { obsPackShape(c, (int32_t)(((int64_t)1 << 31) / 72 + 1), 8); }, "n_rows * H*W >= 2^31");
        want(-EINVAL, [&] { obsPackShape(c, 1, 0); }, "cap 0");
        want(-EINVAL, [&] { obsPackShape(c, 1, 73); }, "cap H*W + 1");
        HandleConfig big = c;
        big.HW = OBS_MAX_CELLS + 1;
        want(-ENOTSUP, [&] { obsPackShape(big, 1, 8); }, "more cells than a cell number holds");
        ObsPackParams P = obsPackShape(c, 4, 8);
        const int32_t* in = (const int32_t*)buf;
        const uint8_t* bytes = (const uint8_t*)buf;
        want(0, [&] { obsPackBuffers(P, in, buf); }, "buffers");
        want(-EINVAL, [&] { obsPackBuffers(P, nullptr, buf); }, "null obs");
        want(-EINVAL, [&] { obsPackBuffers(P, in, nullptr); }, "null out");
        want(-EINVAL, [&] { obsPackBuffers(P, in, (uint32_t*)(bytes + 2)); }, "misaligned out");
        want(0, [&] { obsPackedSource(P, buf, 4, nullptr, buf, 16); }, "source");
        want(0, [&] { obsPackedSource(P, buf, 1, in, buf, 4); }, "one packed row through an index");
        want(-EINVAL, [&] { obsPackedSource(P, nullptr, 4, nullptr, buf, 4); }, "null packed");
        want(-EINVAL, [&] { obsPackedSource(P, buf, 4, nullptr, nullptr, 4); }, "null out");
        want(-EINVAL, [&] { obsPackedSource(P, buf, 0, in, buf, 4); }, "no packed rows");
        want(-EINVAL, [&] { obsPackedSource(P, buf, 3, nullptr, buf, 4); }, "fewer packed rows than rows, no index");
        want(-EINVAL, [&] { obsPackedSource(P, buf, 4, nullptr, bytes + 4, 16); }, "one-hot out not 16-byte aligned");
        want(-EINVAL, [&] { obsPackedSource(P, buf, 4, (const int32_t*)(bytes + 1), buf, 4); }, "misaligned index");
        std::printf("packed observation rows: %d argument sets accepted, %d refused with an error code\n", passed, refused);
    }
    if (g_bad) std::printf("%d check(s) FAILED\n", g_bad);
    else std::printf("clean\n");
    return g_bad ? 1 : 0;
}
