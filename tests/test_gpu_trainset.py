"""The training-set builder on the GPU: addnoise_batch / sea_addnoise bit for bit the numpy model (tests/addnoise_model.py:
in-order float sums, gain, the defined float -> short conversion), trainset_batch equal to its parts, make_trainset
independent of its chunks, the rejections, and the file tool bin/enhance_extract_subband."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import addnoise_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "speech_enhancement_amd", "host", "bin", "enhance_extract_subband")


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def setup():
    """Inputs, the model's results and one trainset_batch run with the noisy subbands; nothing here is modified by a test."""
    import speech_enhancement_amd as sea
    torch = _torch()
    recs, cs = M.recordings(), M.cases()
    src, base = M.noise_layout(recs)
    want = [M.addnoise(c["clean"], M.stretch(recs, c), c["db"]) for c in cs]
    batch = sea.PackedBatch.from_arrays([c["clean"] for c in cs])
    start = np.array([base[c["rec"]] + c["off"] for c in cs], np.int64)
    db = np.array([c["db"] for c in cs], np.int32)
    full = sea.trainset_batch(batch, src, start, db, window=1, noisy_subband=True)
    torch.cuda.synchronize()
    return dict(recs=recs, cases=cs, src=src, start=start, db=db, want=want, batch=batch, full=full)


def _check_audio(S, res, what):
    batch, cs, want = S["batch"], S["cases"], S["want"]
    sums, gain = res["sums"].cpu().numpy(), res["gain"].cpu().numpy()
    scaled, noisy = batch.split(res["noise_scaled"]), batch.split(res["noisy"])
    for u, (c, w) in enumerate(zip(cs, want)):
        tag = f"{what} utt {u} ({c['tag']})"
        print(tag, "sums", sums[u], w["sums"], "gain", gain[u], w["gain"],
              "scaled differ", int((scaled[u] != w["scaled"]).sum()), "noisy differ", int((noisy[u] != w["noisy"]).sum()))
        assert sums[u].tobytes() == w["sums"].tobytes(), tag
        assert np.float32(gain[u]).tobytes() == np.float32(w["gain"]).tobytes(), tag
        assert np.array_equal(scaled[u], w["scaled"]), tag
        assert np.array_equal(noisy[u], w["noisy"]), tag


def test_inputs_take_the_special_paths(setup):
    cs, want = setup["cases"], setup["want"]
    by = {c["tag"]: w for c, w in zip(cs, want)}
    assert by["silent clean"]["gain"] == 0.0 and not by["silent clean"]["scaled"].any()
    assert np.isinf(by["silent noise"]["gain"]) and not by["silent noise"]["scaled"].any()
    assert np.array_equal(by["silent noise"]["noisy"], cs[5]["clean"])
    assert int((np.abs(by["wrap"]["prod"]) >= 32768.0).sum()) > 0


def test_addnoise_batch_is_the_model_bit_for_bit(setup):
    import speech_enhancement_amd as sea
    res = sea.addnoise_batch(setup["batch"], setup["src"], setup["start"], setup["db"])
    _torch().cuda.synchronize()
    _check_audio(setup, res, "addnoise_batch")
    # the pad samples of the packed layout are zero, as PackedBatch.from_arrays leaves them in its input
    pad = np.ones(setup["batch"].total, bool)
    for o, L in zip(setup["batch"].host_offsets, setup["batch"].host_lengths):
        pad[o:o + L] = False
    assert not res["noise_scaled"].cpu().numpy()[pad].any() and not res["noisy"].cpu().numpy()[pad].any()


def test_addnoise_host_form_is_the_model_bit_for_bit(setup):
    import speech_enhancement_amd as sea
    for u in (1, 5, 6, 8):
        c, w = setup["cases"][u], setup["want"][u]
        scaled, noisy, sums, gain = sea.addnoise(c["clean"], M.stretch(setup["recs"], c), c["db"])
        assert sums.tobytes() == w["sums"].tobytes() and np.float32(gain).tobytes() == np.float32(w["gain"]).tobytes()
        assert np.array_equal(scaled, w["scaled"]) and np.array_equal(noisy, w["noisy"])


def test_trainset_batch_audio_is_the_model_bit_for_bit(setup):
    _check_audio(setup, setup["full"], "trainset_batch")


def test_trainset_batch_is_its_parts(setup):
    """Each subband set is subband_batch of the corresponding signal and the IRM irm_target_batch of (clean, SCALED noise):
    the same kernels on the same inputs, so bit for bit."""
    import speech_enhancement_amd as sea
    torch = _torch()
    batch, full = setup["batch"], setup["full"]

    def as_batch(data):
        return sea.PackedBatch(data, batch.offsets, batch.lengths, batch.order, batch.host_offsets, batch.host_lengths)
    sc = sea.subband_batch(batch)
    sn = sea.subband_batch(as_batch(full["noise_scaled"]))
    sy = sea.subband_batch(as_batch(full["noisy"]))
    irm = sea.irm_target_batch(batch, sc, sn, 1)
    torch.cuda.synchronize()
    assert torch.equal(full["sub_clean"], sc) and torch.equal(full["sub_noise"], sn) and torch.equal(full["sub_noisy"], sy)
    a, b = full["irm"].data.cpu().numpy(), irm.data.cpu().numpy()
    assert a.shape == b.shape and a.tobytes() == b.tobytes()
    assert np.array_equal(full["irm"].host_row_offsets, irm.host_row_offsets)


def test_trainset_batch_irm_vs_oracle(setup, oracle):
    """Against the oracle's subbands of the clean signal and of the MODEL's scaled noise: |delta| <= irm_cases.IRM_TOL where the
    oracle is not NaN (test_irm_target_vs_oracle's tolerance, derived in tests/test_irm_cpu.py), NaN positions equal."""
    from tests.irm_cases import IRM_TOL
    full, want = setup["full"], setup["want"]
    got_all = full["irm"].data.cpu().numpy()
    worst = 0.0
    for u, c in enumerate(setup["cases"]):
        ref = oracle.irm_target(oracle.subband64(c["clean"]), oracle.subband64(want[u]["scaled"]), 1)
        got = got_all[full["irm"].host_row_offsets[u]: full["irm"].host_row_offsets[u] + full["irm"].host_rows[u]]
        assert got.shape == ref.shape
        ok = ~np.isnan(ref)
        assert np.array_equal(np.isnan(got), ~ok), f"utt {u}: NaN positions"
        if ok.any():
            worst = max(worst, float(np.abs(got[ok] - ref[ok]).max()))
    print("IRM max |delta| vs oracle", worst)
    assert worst <= IRM_TOL


def test_trainset_batch_without_the_noisy_subbands(setup):
    import speech_enhancement_amd as sea
    torch = _torch()
    full = setup["full"]
    res = sea.trainset_batch(setup["batch"], setup["src"], setup["start"], setup["db"], window=1, noisy_subband=False)
    torch.cuda.synchronize()
    assert res["sub_noisy"] is None
    for k in ("noise_scaled", "noisy", "sums", "gain", "sub_clean", "sub_noise"):
        assert res[k].cpu().numpy().tobytes() == full[k].cpu().numpy().tobytes(), k
    assert res["irm"].data.cpu().numpy().tobytes() == full["irm"].data.cpu().numpy().tobytes()


def _host_plan(S):
    cs = S["cases"]
    return ([c["clean"] for c in cs], S["recs"], np.array([c["rec"] for c in cs], np.int32),
            np.array([c["off"] for c in cs], np.int64), S["db"])


def test_make_trainset_does_not_depend_on_the_chunks(setup, monkeypatch):
    import speech_enhancement_amd as sea
    cl, recs, rec, off, db = _host_plan(setup)
    kw = dict(window=1, want_noise_scaled=True, want_subbands=True, noisy_subband=True)
    monkeypatch.delenv("SEA_TRAINSET_SCRATCH_MB", raising=False)
    one = sea.make_trainset(cl, recs, rec, off, db, **kw)
    assert one["chunks"] == 1
    # three sets: 390 B per sample; 5 MB hold 13 000 samples, the list has 53 000 and one utterance of 33 001 (a chunk of its own)
    monkeypatch.setenv("SEA_TRAINSET_SCRATCH_MB", "5")
    cut = sea.make_trainset(cl, recs, rec, off, db, **kw)
    assert cut["chunks"] >= 3, cut["chunks"]
    for k in ("noisy", "irm", "noise_scaled", "sub_clean", "sub_noise", "sub_noisy"):
        for u, (a, b) in enumerate(zip(one[k], cut[k])):
            assert a.tobytes() == b.tobytes(), (k, u)
    # ... and is the device pipeline's result
    full, batch = setup["full"], setup["batch"]
    irm_all = full["irm"].data.cpu().numpy()
    sub_all = full["sub_clean"].cpu().numpy()
    for u, w in enumerate(setup["want"]):
        assert np.array_equal(one["noisy"][u], w["noisy"]) and np.array_equal(one["noise_scaled"][u], w["scaled"])
        r0, nr = full["irm"].host_row_offsets[u], full["irm"].host_rows[u]
        assert one["irm"][u].tobytes() == irm_all[r0:r0 + nr].tobytes()
        L, o = int(batch.host_lengths[u]), int(batch.host_offsets[u])
        pitch = (L + 7) // 8 * 8
        assert np.array_equal(one["sub_clean"][u], sub_all[o * 64:o * 64 + 64 * pitch].reshape(64, pitch)[:, :L])
    # the optional outputs left out: the required ones are unchanged
    lean = sea.make_trainset(cl, recs, rec, off, db, window=1)
    assert lean["sub_clean"] is None and lean["noise_scaled"] is None
    for k in ("noisy", "irm"):
        for a, b in zip(one[k], lean[k]):
            assert a.tobytes() == b.tobytes()


def test_rejections_leave_the_outputs_alone(setup):
    import speech_enhancement_amd as sea
    from speech_enhancement_amd import _lib
    torch = _torch()
    lib = sea.load()
    recs = setup["recs"]
    short = [np.ones(319, np.int16) * 100]
    # host entry point: L = 319, and an offset one past the last that fits
    for clean, off in ((short, 0), ([setup["cases"][1]["clean"]], len(recs[1]) - 477 + 1), ([setup["cases"][1]["clean"]], -1)):
        n = 1
        noisy = [np.full(len(clean[0]), 77, np.int16)]
        irm = [np.full((4, 64), 7.0, np.float32)]
        ptrs = lambda arrs: (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        lens = (ctypes.c_long * 1)(len(clean[0]))
        nlens = (ctypes.c_long * len(recs))(*[len(r) for r in recs])
        rc = lib.sea_trainset_utterances(ptrs(clean), lens, n, ptrs(recs), nlens, len(recs), (ctypes.c_int * 1)(1),
                                         (ctypes.c_long * 1)(off), (ctypes.c_int * 1)(0), 1, ptrs(noisy), ptrs(irm), None, None,
                                         None, None)
        assert rc != 0 and lib.sea_last_error()
        assert (noisy[0] == 77).all() and (irm[0] == 7.0).all()
    with pytest.raises(_lib.SeaError):
        sea.make_trainset(short, recs, [0], [0], np.array([0], np.int32))
    # device entry point: the length check comes before any launch
    batch = sea.PackedBatch.from_arrays(short)
    dev = batch.data.device
    src = torch.from_numpy(setup["src"]).to(dev)
    z64 = torch.zeros(1, dtype=torch.int64, device=dev)
    snr = torch.ones(1, dtype=torch.float32, device=dev)
    outs = [torch.full_like(batch.data, 77) for _ in range(2)]
    subs = [torch.full((batch.total * 64,), 77, dtype=torch.int16, device=dev) for _ in range(2)]
    irm = torch.full((1, 64), 7.0, dtype=torch.float32, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib.sea_trainset_batch(p(batch.data), p(batch.offsets), p(batch.lengths), p(src), p(z64), p(snr), p(outs[0]), p(outs[1]),
                                None, None, p(subs[0]), p(subs[1]), None, p(z64), p(irm), 1, None, 1, None)
    torch.cuda.synchronize()
    assert rc != 0 and b"319" in lib.sea_last_error()
    assert all(bool((t == 77).all()) for t in outs + subs) and bool((irm == 7.0).all())
    with pytest.raises(ValueError):
        sea.trainset_batch(batch, setup["src"], [0], np.array([0], np.int32))
    with pytest.raises(ValueError):
        sea.addnoise_batch(setup["batch"], setup["src"][:100], setup["start"], setup["db"])


# ---------------------------------------------------------------------------------------------------------------------
# the file tool
# ---------------------------------------------------------------------------------------------------------------------
def _write_wav(path, x, fs=16000):
    import wave
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(fs)
        w.writeframes(np.ascontiguousarray(x, "<i2").tobytes())


def _read_wav(path):
    import wave
    with wave.open(str(path), "rb") as w:
        assert w.getnchannels() == 1 and w.getsampwidth() == 2
        return np.frombuffer(w.readframes(w.getnframes()), "<i2").astype(np.int16)


def _tool_tree(root, name, func="train"):
    out = root / name
    for d in ("noisy", "sub_pure", "sub_noise", "sub_noisy"):
        (out / d).mkdir(parents=True)
    values = [func, f"{root}/in/", f"{root}/list.txt"] + [f"{root}/noise{k}.wav" for k in range(4)] + ["-5", f"{out}/", "noisy/",
              "sub_pure/", "sub_noise/", "sub_noisy/", "ibm/", "irm/", "sirm/", "mfcc/", "acf/", "wiener/", "Log.txt"]
    keys = ["func", "purewavDictionary", "purewavlist", "noisepath1", "noisepath2", "noisepath3", "noisepath4", "addnoisedB",
            "outputDictionary", "save_noisy_dir", "save_subband_pure_wav_dir", "save_subband_noise_wav_dir",
            "save_subband_noisy_wav_dir", "save_subband_noisy_IBM_dir", "save_subband_noisy_IRM_dir",
            "save_subband_noisy_sIBM_dir", "save_subband_noisy_MFCC", "save_subband_noisy_ACF", "save_subband_noisy_Wiener", "log"]
    cfg = root / f"{name}.cfg"
    cfg.write_text("".join(f"{k}= {v}\n" for k, v in zip(keys, values)))
    return cfg, out


def _run_tool(*args):
    r = subprocess.run([TOOL] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    return r


def _plan_of(log):
    plan = {}
    for line in open(log):
        t = line.split()
        if len(t) == 4:
            try:
                plan[t[0]] = (int(t[1]), int(t[2]), int(t[3]))
            except ValueError:
                pass
    return plan


def test_file_tool(tmp_path):
    import speech_enhancement_amd as sea
    from speech_enhancement_amd import corpus
    assert os.path.exists(TOOL), "build with make -C speech_enhancement_amd/host"
    ids = [f"utt{k}" for k in range(5)]
    lens = [1600, 2400, 3205, 4800, 3360]
    clean = [corpus.synth_utterance(u, L) for u, L in zip((221, 222, 223, 224, 226), lens)]
    noises = [(corpus.synth_utterance(320 + k, n).astype(np.int32) // 3).astype(np.int16)
              for k, n in enumerate((12000, 9000, 10000, 8000))]
    (tmp_path / "in").mkdir()
    for i, x in zip(ids, clean):
        _write_wav(tmp_path / "in" / f"{i}.wav", x)
    for k, x in enumerate(noises):
        _write_wav(tmp_path / f"noise{k}.wav", x)
    (tmp_path / "list.txt").write_text("".join(f"{i}\n" for i in ids))

    cfg1, out1 = _tool_tree(tmp_path, "run1")
    r = _run_tool(cfg1, "--seed", "1")
    assert r.returncode == 0, r.stderr
    plan = _plan_of(out1 / "Log.txt")
    assert sorted(plan) == ids
    rec = np.array([plan[i][0] for i in ids], np.int32)
    off = np.array([plan[i][1] for i in ids], np.int64)
    db = np.array([plan[i][2] for i in ids], np.int32)
    want = sea.make_trainset(clean, noises, rec, off, db, window=1)
    for k, i in enumerate(ids):
        model = M.addnoise(clean[k], noises[rec[k]][off[k]:off[k] + lens[k]], int(db[k]))
        assert np.array_equal(_read_wav(out1 / "noisy" / f"{i}_noisy.wav"), model["noisy"]), i
    with open(out1 / "IRM.sIRM") as f:
        mats = list(corpus.read_mask_text(f))
    assert [m[0] for m in mats] == [f"{i}_noisy" for i in ids]
    for k, (_, m) in enumerate(mats):
        printed = np.array([[float("%.7f" % v) for v in row] for row in want["irm"][k]], np.float32)
        assert m.shape == printed.shape and np.array_equal(m, printed, equal_nan=True), ids[k]
    for d, tail in (("sub_pure", ""), ("sub_noise", "_noise"), ("sub_noisy", "_noisy")):
        assert len(os.listdir(out1 / d)) == 64 * len(ids)
        assert all((out1 / d / f"{i}{tail}_{ch}.wav").exists() for i in ids for ch in range(64))
    sub = sea.subbband(clean[2])
    for ch in range(64):
        assert np.array_equal(_read_wav(out1 / "sub_pure" / f"{ids[2]}_{ch}.wav"), sub[ch]), ch

    # the same plan from the Log, without the subband files: the same bytes
    cfg2, out2 = _tool_tree(tmp_path, "run2")
    r = _run_tool(cfg2, "--no-subband-wavs", "--plan", out1 / "Log.txt")
    assert r.returncode == 0, r.stderr
    assert _plan_of(out2 / "Log.txt") == plan
    for d in ("sub_pure", "sub_noise", "sub_noisy"):
        assert os.listdir(out2 / d) == []
    assert (out2 / "IRM.sIRM").read_bytes() == (out1 / "IRM.sIRM").read_bytes()
    for i in ids:
        assert (out2 / "noisy" / f"{i}_noisy.wav").read_bytes() == (out1 / "noisy" / f"{i}_noisy.wav").read_bytes()


def test_file_tool_func_test_and_sample_rates(tmp_path):
    """func = test (the reference's inverted switch: mixing OFF): the noisy file is a copy of the clean one, the noise subbands
    are those of the UNSCALED stretch the plan names, the noisy subbands those of the clean signal, and no IRM is written.  An
    utterance at another sample rate than the noise files is reported and skipped, not mixed."""
    import speech_enhancement_amd as sea
    from speech_enhancement_amd import corpus
    ids = ["a", "b", "other_rate"]
    clean = [corpus.synth_utterance(231, 1600), corpus.synth_utterance(232, 2005), corpus.synth_utterance(233, 1600)]
    noises = [(corpus.synth_utterance(330 + k, 6000).astype(np.int32) // 3).astype(np.int16) for k in range(4)]
    (tmp_path / "in").mkdir()
    for i, x in zip(ids, clean):
        _write_wav(tmp_path / "in" / f"{i}.wav", x, 8000 if i == "other_rate" else 16000)
    for k, x in enumerate(noises):
        _write_wav(tmp_path / f"noise{k}.wav", x)
    (tmp_path / "list.txt").write_text("".join(f"{i}\n" for i in ids))

    cfg, out = _tool_tree(tmp_path, "copy", func="test")
    r = _run_tool(cfg, "--seed", "3")
    assert r.returncode != 0 and "other_rate" in r.stderr and "8000" in r.stderr, r.stderr
    plan = _plan_of(out / "Log.txt")
    assert sorted(plan) == ["a", "b"]
    assert not (out / "IRM.sIRM").exists()
    assert sorted(os.listdir(out / "noisy")) == ["a_noisy.wav", "b_noisy.wav"]
    for k, i in enumerate(ids[:2]):
        assert np.array_equal(_read_wav(out / "noisy" / f"{i}_noisy.wav"), clean[k])
        rec, off, _ = plan[i]
        sub_c, sub_n = sea.subbband(clean[k]), sea.subbband(noises[rec][off:off + len(clean[k])])
        for ch in (0, 17, 63):
            assert np.array_equal(_read_wav(out / "sub_pure" / f"{i}_{ch}.wav"), sub_c[ch])
            assert np.array_equal(_read_wav(out / "sub_noise" / f"{i}_noise_{ch}.wav"), sub_n[ch])
            assert np.array_equal(_read_wav(out / "sub_noisy" / f"{i}_noisy_{ch}.wav"), sub_c[ch])
    log = (out / "Log.txt").read_text()
    assert log.count("subband") == 2 and "single_IBM" not in log

    # with mixing on, the same list: the utterance at the other rate is skipped there too, the others are mixed
    cfg2, out2 = _tool_tree(tmp_path, "mixed")
    r = _run_tool(cfg2, "--no-subband-wavs", "--plan", out / "Log.txt")
    assert r.returncode != 0 and "other_rate" in r.stderr
    assert sorted(os.listdir(out2 / "noisy")) == ["a_noisy.wav", "b_noisy.wav"]
    log2 = (out2 / "Log.txt").read_text()
    assert log2.count("subband") == 2 and log2.count("single_IBM") == 2      # once per utterance, as the reference logs them
    # noise files of two rates are refused as a whole
    _write_wav(tmp_path / "noise2.wav", noises[2], 8000)
    r = _run_tool(cfg2, "--no-subband-wavs", "--seed", "3")
    assert r.returncode != 0 and "noise2.wav" in r.stderr
