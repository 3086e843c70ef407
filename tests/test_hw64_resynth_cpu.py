"""The Hu-Wang resynthesis at 16 kHz on the 64-channel bank without a GPU: the numpy model (tests/hw64_resynth_model.py) against
what the reference's own resynthesis(), compiled against the 64-band header, produced (tests/golden/hw64_resynth_golden.npz,
tools/gen_hw64_resynth_golden.py), bit for bit on every case; the library's host tables against the model's; the text writer
against the reference's file; the new symbols, none of which takes a stream; and the plan that cuts a list of utterances into
chunks, held to its stated properties."""
import ctypes
import os
import re
import zlib

import numpy as np
import pytest

from tests import hw64_am_model as AM
from tests import hw64_model as M
from tests import hw64_resynth_model as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sea_mi355x.h")
NEW_SYMBOLS = ("sea_hw64_resynth_tables_host", "sea_hw64_resynth", "sea_hw64_enhance", "sea_hw64_resynth_utterances",
               "sea_hw64_enhance_utterances", "sea_hw64_enhance_plan", "sea_hw64_enhance_last_chunks",
               "sea_hw64_enhance_last_resynth_ms")
NCH, HOP = 64, 160


@pytest.fixture(scope="module")
def golden():
    return RM.load_golden()


@pytest.fixture(scope="module")
def cases():
    return RM.reference_cases(AM.load_golden())


def test_the_cases_are_the_fixtures_and_every_mask_is_in_bounds(golden, cases):
    assert len(cases) == len(RM.AUDIO_CASES) + len(RM.HAND_INPUTS) * len(RM.HAND_MASKS) == 19
    assert len([k for k in golden if k.startswith("out_")]) == 19
    for k, (x, mask) in cases.items():
        assert mask.shape == (len(x) // HOP, NCH)
        assert np.array_equal(golden[f"mask_{k}"], mask.astype(np.int8)), k
        assert golden[f"out_{k}"].shape == x.shape and golden[f"out_{k}"].dtype == np.float32, k
        assert RM.in_bounds(mask > 0, len(x)), k
    assert len(RM.hand_input("w4096")) % HOP == 96 and len(RM.hand_input("t3200")) == 3200
    assert 160 * 19 + 159 == len(RM.hand_input("t3200")) - 1
    # no drop rule on this bank: a mask whose last row is set is in bounds at every length, and such masks are in the fixture
    for L in (160, 161, 319, 320, 3203):
        m = np.zeros((L // HOP, NCH), bool)
        m[-1] = True
        assert RM.in_bounds(m, L)
    for i in RM.HAND_INPUTS:
        assert golden[f"mask_h_{i}_last"][-1].all() and golden[f"mask_h_{i}_ones"][-1].all()
    assert golden["mask_h_w4096_single"].sum() == 1 and golden["mask_h_w4096_single"][:, 47].sum() == 1
    assert golden["mask_h_t3200_high"][:, 32:].all() and not golden["mask_h_t3200_high"][:, :32].any()


def test_model_equals_the_reference_on_every_case(golden, cases):
    for k, (x, mask) in cases.items():
        got = RM.resynth_input(RM.case_input(k), mask)
        assert M.same_bits(got, golden[f"out_{k}"]), f"{k}: the model is not the reference's resynthesis"
        assert np.abs(got).max() > 100, k


def test_soft_mask_is_its_positive_part_at_threshold_zero(golden):
    for i in RM.HAND_INPUTS:
        soft = RM.hand_mask("soft", len(RM.hand_input(i)) // HOP)
        assert set(np.unique(soft)) == {np.float32(0), np.float32(0.3), np.float32(0.7)}
        assert M.same_bits(RM.resynth_input(i, soft), golden[f"out_h_{i}_soft"])
        assert not M.same_bits(RM.resynth_input(i, soft, 0.5), golden[f"out_h_{i}_soft"])


def test_weights_follow_the_window_without_quirk_or_drop():
    up, down = RM.ola_tables()
    assert up.shape == down.shape == (160,) and up[0] == 0 and down[0] == 1 and 0 < down[159] < 1e-3 and (np.diff(down) < 0).all()
    # one set unit at frame 3 of 6: up on [320, 480), down on [480, 640), nothing else
    m = np.zeros((6, NCH), bool)
    m[3, 47] = True
    w = RM.weights(m, 1000)
    assert M.same_bits(w[47, 320:480], up.astype(np.float32)) and M.same_bits(w[47, 480:640], down.astype(np.float32))
    assert not w[47, :320].any() and not w[47, 640:].any() and not np.delete(w, 47, axis=0).any()
    # frame 0 has no rising half; the last frame ends at 160 F - 1 and the tail [160 F, L) stays 0
    m[:] = False
    m[0, 0] = m[5, 0] = True
    w = RM.weights(m, 1000)
    assert M.same_bits(w[0, :160], down.astype(np.float32)) and M.same_bits(w[0, 800:960], down.astype(np.float32))
    assert M.same_bits(w[0, 640:800], up.astype(np.float32)) and not w[0, 960:].any() and not w[0, 160:640].any()
    # two frames in a row: the sample 160 k + o sums down[o] from frame k, then up[o] from frame k + 1, each rounded to float
    m[:] = False
    m[2:4, 63] = True
    w = RM.weights(m, 1000)
    want = (down.astype(np.float32).astype(np.float64) + up).astype(np.float32)
    assert M.same_bits(w[63, 320:480], want)


def test_host_tables_equal_the_models():
    import speech_enhancement_amd as sea
    t = sea.hw64_resynth_tables()
    up, down = RM.ola_tables()
    assert M.same_bits(t["up"], up) and M.same_bits(t["down"], down)
    w = RM.weight_table()
    assert t["w"].shape == w.shape == (160, 4) and M.same_bits(t["w"], w), "the 640 weights"
    assert not w[:, 0].any() and M.same_bits(w[:, 1], down.astype(np.float32)) and M.same_bits(w[:, 2], up.astype(np.float32))
    assert (np.abs(w[:, 3] - 1) < 1e-6).all(), "a raised cosine: two neighbouring set frames add up to one"
    from speech_enhancement_amd import _lib
    assert _lib.load().sea_hw64_resynth_tables_host(None, None, None) == 0


def test_text_writer_gives_the_references_bytes(golden, cases, tmp_path):
    from speech_enhancement_amd import _lib
    lib = _lib.load()
    for k in cases:
        out = golden[f"out_{k}"]
        path = tmp_path / f"{k}.txt"
        assert lib.sea_hw25_resynth_text_write(str(path).encode(), out.ctypes.data_as(ctypes.c_void_p), len(out)) == 0
        got = path.read_bytes()
        assert zlib.crc32(got) & 0xFFFFFFFF == int(golden[f"text_crc_{k}"]), k
        assert got == RM.text(out), k
        if k in RM.TEXT_CASES:
            assert got == golden[f"text_{k}"].tobytes(), k
    assert all(f"text_{k}" in golden for k in RM.TEXT_CASES)


def test_new_symbols_are_declared_bound_and_take_no_stream():
    import speech_enhancement_amd as sea
    from speech_enhancement_amd import _lib
    from tests import stream_cases as S
    raw = ctypes.CDLL(sea.LIB_PATH)
    header = open(HEADER).read()
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), f"{name} is not exported by the library"
        assert name in _lib.PROTOTYPES, f"{name} has no prototype"
        assert f"{name}(" in header, f"{name} is not declared in include/sea_mi355x.h"
    for name in ("sea_hw64_resynth", "sea_hw64_enhance", "sea_hw64_resynth_tables_host"):
        assert _lib.PROTOTYPES[name] == _lib.PROTOTYPES[name.replace("hw64", "hw25")], f"{name} does not mirror its 25-band namesake"
    proto = lambda name: re.sub(r"\s+", " ", re.search(name + r"\(([^;]*)\);", header).group(1))  # noqa: E731
    for name in ("sea_hw64_resynth", "sea_hw64_enhance"):
        assert proto(name) == proto(name.replace("hw64", "hw25")), f"{name}: the header's parameters are not its namesake's"
    # no exported device-pointer form arrives with this feature: the table of stream-taking prototypes is what it was
    streams = S.stream_prototypes()
    assert len(streams) == 44 and not [n for n in streams if "hw64_resynth" in n or "hw64_enhance" in n]
    for name in NEW_SYMBOLS:
        assert not re.search(name + r"\([^;]*\bstream\b[^;]*\);", header), f"{name} takes a stream"
    assert "sea_hw64_resynth_batch(" not in header and "sea_hw64_enhance_batch(" not in header
    assert b"hw64_resynth_kernel" in open(sea.LIB_PATH, "rb").read()
    for name in ("hw64_resynth", "hw64_enhance", "hw64_resynth_utterances", "hw64_enhance_utterances", "hw64_resynth_tables",
                 "hw64_enhance_plan"):
        assert callable(getattr(sea, name))


# ---- the plan ------------------------------------------------------------------------------------------------------------------
def _bound(lib, lengths, resynth_only):
    """a chunk's footprint as include/sea_mi355x.h states it"""
    s = sum((L + 7) // 8 * 8 for L in lengths)
    r = sum(L // HOP for L in lengths)
    n = len(lengths)
    work = 768 * s if resynth_only else int(lib.sea_hw64_ibm_scratch_bytes(s, r, n))
    return work + 10 * s + 260 * r + 32 * n


@pytest.mark.parametrize("resynth_only", [False, True])
def test_plan_properties(resynth_only):
    import speech_enhancement_amd as sea
    from speech_enhancement_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(7)
    lengths = [int(v) for v in rng.integers(0, 70000, 40)] + [0, 159, 160, 150000, 3203]
    n = len(lengths)
    one = _bound(lib, [64000], resynth_only)
    seen = set()
    for budget in (0, 1, one, 3 * one, 10 * one + 12345, _bound(lib, lengths, resynth_only) - 1, _bound(lib, lengths, resynth_only), 1 << 60):
        cuts = sea.hw64_enhance_plan(lengths, budget, resynth_only)
        # the cuts partition the list in order
        assert cuts[0] == 0 and cuts[-1] == n and (np.diff(cuts) > 0).all(), budget
        for a, b in zip(cuts[:-1], cuts[1:]):
            # a chunk's bound holds unless it has one utterance
            assert b - a == 1 or _bound(lib, lengths[a:b], resynth_only) <= budget, (budget, a, b)
            # greedy: the next utterance would not have fitted
            assert b == n or _bound(lib, lengths[a:b + 1], resynth_only) > budget, (budget, a, b)
        seen.add(len(cuts) - 1)
    assert len(sea.hw64_enhance_plan(lengths, 0, resynth_only)) - 1 == n, "a budget of 0 gives one utterance per chunk"
    assert len(sea.hw64_enhance_plan(lengths, 1 << 60, resynth_only)) - 1 == 1, "a huge budget gives one chunk"
    assert len(sea.hw64_enhance_plan(lengths, _bound(lib, lengths, resynth_only) - 1, resynth_only)) - 1 == 2
    assert len(seen) >= 5
    # the count alone, an empty list, a refused length
    arr = (ctypes.c_long * n)(*lengths)
    assert lib.sea_hw64_enhance_plan(arr, n, 3 * one, int(resynth_only), None) == len(sea.hw64_enhance_plan(lengths, 3 * one, resynth_only)) - 1
    assert lib.sea_hw64_enhance_plan(None, 0, 0, 0, None) == 0 and list(sea.hw64_enhance_plan([], 5, resynth_only)) == [0]
    assert lib.sea_hw64_enhance_plan((ctypes.c_long * 2)(100, -1), 2, 0, 0, None) == -1
    with pytest.raises(sea.SeaError):
        sea.hw64_enhance_plan([100, -1], 0)


def test_the_estimators_chunks_are_small_at_this_bank():
    """about 200 MB of scratch per four-second utterance: why a list has to be cut"""
    from speech_enhancement_amd import _lib
    lib = _lib.load()
    per = _bound(lib, [64000], False)
    assert 150e6 < per < 300e6
    assert _bound(lib, [64000], True) < per / 3
