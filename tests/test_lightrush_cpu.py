"""CPU-side checks of the native LightRush's boundary: the bot-kind names, the enum of include/mrts.h against the
Python binding, and the state-block size of handles without a LightRush game, which must not have moved (the
specialised self-play kernels compile it in)."""
import os
import re

import pytest

from microrts_amd import _lib
from microrts_amd.vec_client import _bot_kind
from tests.headers import internal_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bot_kind_names():
    for name in ("LightRush", "lightRushAI", "light_rush"):
        assert _bot_kind(name) == 2 == _lib.MRTS_BOT_LIGHT_RUSH

    class LightRush:  # an object or a class named like the Java class (JPype proxies)
        pass

    assert _bot_kind(LightRush()) == 2 and _bot_kind(LightRush) == 2
    assert _bot_kind("PassiveAI") == 0 and _bot_kind("RandomBiasedAI") == 1
    for other in ("WorkerRush", "HeavyRush", "RangedRush", "lightrush", "LightRushAI"):
        with pytest.raises(NotImplementedError, match="PassiveAI / RandomBiasedAI / LightRush"):
            _bot_kind(other)


def test_header_enum_matches_the_binding():
    txt = open(os.path.join(ROOT, "include", "mrts.h")).read()
    m = re.search(r"enum\s*\{\s*(MRTS_BOT_[^}]*)\}", txt)
    assert m, "no MRTS_BOT_* enum in include/mrts.h"
    got = {k: int(v) for k, v in re.findall(r"(MRTS_BOT_\w+)\s*=\s*(\d+)", m.group(1))}
    assert got == {"MRTS_BOT_PASSIVE": _lib.MRTS_BOT_PASSIVE, "MRTS_BOT_RANDOM_BIASED": _lib.MRTS_BOT_RANDOM_BIASED,
                   "MRTS_BOT_LIGHT_RUSH": _lib.MRTS_BOT_LIGHT_RUSH}
    assert got["MRTS_BOT_LIGHT_RUSH"] == 2


@pytest.mark.parametrize("cap,hw", [(128, 64), (320, 256), (320, 1024), (1280, 1024)], ids=["c2", "c3", "c5", "32x32-full"])
def test_state_words_without_lightrush_is_unchanged(cap, hw):
    """stateWords(CAP, HW) is what it was before the bot memory existed: header, 7 unit arrays, the two previous
    mask row sets, the terrain bytes and the 64 forwarded action words; the LightRush memory is a separate
    botWords(CAP), appended only in handles that have a LightRush game."""
    h = internal_header()
    want = 16 + 7 * cap + 2 * ((hw + 31) // 32) + (hw + 3) // 4 + 64
    assert h["stateWords"](cap, hw) == want
    assert {(128, 64): 996, (320, 256): 2400, (320, 1024): 2640}.get((cap, hw), want) == want
    assert h["botWords"](cap) == 2 * (4 + 3 * cap)
    assert h["LR_MAX_CELLS"] == 1024
