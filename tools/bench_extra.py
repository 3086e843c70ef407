#!/usr/bin/env python3
"""tools/bench_extra.py -- measurements of the other hot-path kernels (BASELINE configs[2], [3] and
the CompCeps front-end) on one MI355X.  bench.py stays the headline (NoiseSup, configs[1]); this
script prints one JSON line per workload with the same roofline convention.

    python tools/bench_extra.py [--utts 1024] [--steps 5] [--what resynth,ibm,ceps,rfft]
    python tools/bench_extra.py --what wb --steps 7      # the ETSI wideband (16 kHz) mode, opt-in
    python tools/bench_extra.py --what wbafe --steps 7   # its feature chain (WaveProc, PostProc, VAD), opt-in
    python tools/bench_extra.py --what wbslices --steps 7  # the wideband mode in time slices and its host pipeline, opt-in
    python tools/bench_extra.py --what wbafeslices --steps 7  # its feature chain in time slices and from host buffers, opt-in
    python tools/bench_extra.py --what afeslices --steps 7  # the 8 kHz feature chain in time slices and from host buffers, opt-in
    python tools/bench_extra.py --what cepsslices --steps 7  # NoiseSup + the plain CompCeps in time slices and from host buffers, both rates, opt-in
    python tools/bench_extra.py --what trainset --steps 7  # the training-set builder: mix, subbands, IRM, pipeline and host entry point, opt-in
    python tools/bench_extra.py --what hw25 --steps 5  # the Hu-Wang front half on the 25-channel bank: periphery, correlogram, launch group, opt-in
    python tools/bench_extra.py --what hw64 --steps 3  # the same front half at 16 kHz on the 64-channel bank, opt-in
    python tools/bench_extra.py --what hw25pitch --steps 3  # its initial grouping and pitch tracking beside the correlogram, opt-in
    python tools/bench_extra.py --what hw64pitch --steps 3  # the same stage at 16 kHz on the 64-channel bank, opt-in
    python tools/bench_extra.py --what hw25ibm --steps 3  # its AM stage, final grouping and the whole estimator beside the other stages, opt-in
    python tools/bench_extra.py --what hw64ibm --steps 3  # the same at 16 kHz on the 64-channel bank; also writes profiles/hw64ibm_bench_extra.jsonl, opt-in
    python tools/bench_extra.py --what hw25resynth --steps 3  # its resynthesis alone and audio in / enhanced audio out, beside the estimator and the periphery, opt-in
    python tools/bench_extra.py --what hw64resynth --steps 3  # the same at 16 kHz on the 64-channel bank, through the host-list forms; also writes profiles/hw64resynth_bench_extra.jsonl, opt-in
    python tools/bench_extra.py --what dnn --steps 5  # the DNN mask estimator: cochleagram, every layer (TFLOP/s), the chain, beside the resynthesis alone and hw64_enhance_utterances; also writes profiles/dnn_bench_extra.jsonl, opt-in
    python tools/bench_extra.py --what dnntrain  # its trainer: 200 SGD steps at minibatch 256, 1024 and 4096, every stage (TFLOP/s per GEMM beside the forward layer at the same M), steps/s, an epoch's time; also writes profiles/dnntrain_bench_extra.jsonl, opt-in
    python tools/bench_extra.py --what score --steps 5  # the objective scores: each kernel between device events beside the bytes it reads, the host calls' wall time; also writes profiles/score_bench_extra.jsonl, opt-in
    python tools/bench_extra.py --what stoi --steps 5  # STOI: each kernel between device events, the band kernel's TFLOP/s beside the DNN forward layer's, the host call's wall time; also writes profiles/stoi_bench_extra.jsonl, opt-in
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (build_shard)

HBM_PEAK_GBPS = 8000.0


def timed(fn, steps, warmup=1):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    t0 = time.perf_counter()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / steps
    return wall, float(np.mean([a.elapsed_time(b) for a, b in ev])) / 1e3


def median_ms(fn, steps):
    """device events around every step after one discarded warm-up call: (median, sorted list), in ms"""
    import torch
    fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in ev)
    return t[len(t) // 2], t


def wb_batch(batch, dev):
    """the batch of --what wb and --what wbafe: the corpus plus as many wideband signals of the same lengths"""
    import speech_enhancement_amd as sea
    from speech_enhancement_amd import corpus
    lens = [int(L) for L in batch.host_lengths]
    host = batch.data.cpu().numpy()
    utts = [host[o:o + l] for o, l in zip(batch.host_offsets, lens)] + [corpus.synth_wideband(u, L) for u, L in enumerate(lens)]
    return sea.PackedBatch.from_arrays(utts, dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--what", default="resynth,ibm,subband,ceps,afe,rfft,host")
    args = ap.parse_args()
    import torch
    import speech_enhancement_amd as sea
    from speech_enhancement_amd import corpus
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    what = set(args.what.split(","))
    batch = bench.build_shard(args.utts, 0, dev)
    audio_s = float(np.sum(batch.host_lengths)) / 16000.0

    if what & {"resynth", "ibm"}:
        masks = sea.MaskBatch.from_arrays([corpus.synth_mask(u, int(L)) for u, L in enumerate(batch.host_lengths)], dev)
        hops = int(np.sum((np.asarray(batch.host_lengths) - 320) // 160 + 1))
        scratch = torch.empty(sea.resynth_scratch_elems(batch), dtype=torch.float32, device=dev)
        out = torch.zeros_like(batch.data)
        for name, binary in (("resynth", False), ("ibm", True)):
            if name not in what:
                continue
            wall, ker = timed(lambda: sea.resynth_batch(batch, masks, binary=binary, out=out, scratch=scratch), args.steps)
            alg = hops * 896
            print(json.dumps({
                "metric": f"resynth_64sub_{'IBM' if binary else 'ori'} hop-frames/sec (160-sample hop, 64 bands)",
                "value": hops / wall, "unit": "hop-frames/s", "ms_per_step": wall * 1e3, "rtf": wall / audio_s,
                "config": {"workload": f"BASELINE configs[{3 if binary else 2}]: {args.utts} utterances, 64-band gammatone "
                                       f"analysis/synthesis, {'ideal binary' if binary else 'ratio'} mask", "hop_frames": hops},
                "roofline": {"bound": "hbm", "kernels": "sea::resynth_fused_kernel",
                             "achieved": alg / ker / 1e9, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                             "frac": alg / ker / 1e9 / HBM_PEAK_GBPS, "algorithmic_bytes_per_step": alg,
                             "intermediate_bytes_per_step": int(batch.total) * 64 * 4 * 2,
                             "intermediate_GBps": int(batch.total) * 64 * 4 * 2 / ker / 1e9, "avg_step_ms": ker * 1e3}}),
                  flush=True)

    if "subband" in what:
        out = torch.zeros(batch.total * 64, dtype=torch.int16, device=dev)
        wall, ker = timed(lambda: sea.subband_batch(batch, out=out), args.steps)
        samples = int(np.sum(batch.host_lengths))
        alg = samples * (2 + 128)
        print(json.dumps({
            "metric": "subbband() samples/sec (gammatone + hair cell -> 64 int16 streams)", "value": samples / wall,
            "unit": "samples/s", "ms_per_step": wall * 1e3, "rtf": wall / audio_s,
            "config": {"workload": f"SURVEY 8(f) #1: {args.utts} utterances, 64-channel analysis to 64 int16 streams"},
            "roofline": {"bound": "hbm", "kernel": "sea::subband_kernel", "achieved": alg / ker / 1e9,
                         "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": alg / ker / 1e9 / HBM_PEAK_GBPS,
                         "algorithmic_bytes_per_step": alg, "avg_step_ms": ker * 1e3}}), flush=True)
        del out

    if "irm" in what:   # SURVEY 8(f) #2 on two different subband blocks (as bench.py's also-line)
        sub = torch.zeros(batch.total * 64, dtype=torch.int16, device=dev)
        sub2 = torch.zeros(batch.total * 64, dtype=torch.int16, device=dev)
        keep = batch.data
        batch.data = torch.flip(keep, dims=[0]).contiguous()
        sea.subband_batch(batch, out=sub2)
        batch.data = keep
        sea.subband_batch(batch, out=sub)
        torch.cuda.synchronize()
        wall, ker = timed(lambda: sea.irm_target_batch(batch, sub, sub2), args.steps)
        hops = int(np.sum((np.asarray(batch.host_lengths) - 320) // 160 + 1))
        alg = hops * (2 * 128 * 160 + 256)
        print(json.dumps({
            "metric": "IRM target hop-frames/sec (x 64 channels)", "value": hops / wall, "unit": "hop-frames/s", "ms_per_step": wall * 1e3,
            "config": {"workload": f"SURVEY 8(f) #2: {args.utts} utterances, {hops} frames x 64 channels from two subband blocks"},
            "roofline": {"bound": "hbm", "kernel": "sea::irm_target_kernel", "achieved": alg / ker / 1e9, "peak": HBM_PEAK_GBPS,
                         "unit": "GB/s", "frac": alg / ker / 1e9 / HBM_PEAK_GBPS, "algorithmic_bytes_per_step": alg,
                         "avg_step_ms": ker * 1e3}}), flush=True)
        del sub, sub2

    if "ceps" in what:
        out, f32, first = sea.ns_denoise_batch(batch, want_f32=True)
        torch.cuda.synchronize()
        res = {}

        def run():
            res["c"] = sea.compceps_batch(batch, f32, first)
        wall, ker = timed(run, args.steps)
        n = int(res["c"][2].sum().item())
        alg = n * (320 + 56)
        print(json.dumps({"metric": "CompCeps cepstral frames/sec (from the float NoiseSup stream)", "value": n / wall,
                          "unit": "frames/s", "ms_per_step": wall * 1e3,
                          "config": {"workload": f"{args.utts} utterances, {n} cepstral frames of 14 coefficients"},
                          "roofline": {"bound": "hbm", "kernel": "sea::compceps_kernel", "achieved": alg / ker / 1e9,
                                       "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": alg / ker / 1e9 / HBM_PEAK_GBPS,
                                       "algorithmic_bytes_per_step": alg, "avg_step_ms": ker * 1e3}}), flush=True)

    if "afe" in what:
        # NoiseSup (with speech flags) -> WaveProc -> CompCeps -> PostProc -> VAD + flush
        lib = sea.load()
        n = batch.n_utt
        outb = torch.zeros_like(batch.data)
        f32 = torch.zeros(batch.total, dtype=torch.float32, device=dev)
        first = torch.full((n,), -1, dtype=torch.int32, device=dev)
        onset = torch.zeros(n, dtype=torch.int32, device=dev)
        flags = torch.zeros(batch.total // 8, dtype=torch.uint8, device=dev)
        nfr = np.asarray(batch.host_lengths) // 80
        ccum = np.concatenate(([0], np.cumsum(np.maximum(nfr - 6, 0)))).astype(np.int64)
        fcum = np.concatenate(([0], np.cumsum(nfr + 6))).astype(np.int64)
        tc, tf = int(ccum[-1]), int(fcum[-1])
        fcc = torch.zeros((tc, 14), dtype=torch.float32, device=dev)
        f15 = torch.zeros((tf, 15), dtype=torch.float32, device=dev)
        nfe = torch.zeros(n, dtype=torch.int32, device=dev)
        d_ccum, d_fcum = torch.from_numpy(ccum).to(dev), torch.from_numpy(fcum).to(dev)
        P = lambda t: t.data_ptr()
        st = torch.cuda.current_stream().cuda_stream

        def ns_fd():
            assert lib.sea_ns_denoise_batch_fd(P(batch.data), P(outb), P(f32), P(batch.offsets), P(batch.lengths),
                                               P(batch.order), P(first), P(flags), P(onset), n, st) == 0

        def feats():
            assert lib.sea_afe_features_batch(P(f32), P(flags), P(batch.offsets), P(batch.lengths), P(first), P(onset),
                                              P(d_ccum), tc, P(fcc), None, P(d_fcum), P(f15), P(nfe), None, n, st) == 0
        w1, k1 = timed(ns_fd, args.steps)
        w2, k2 = timed(feats, args.steps)
        emitted = int(nfe.sum().item())
        alg = batch.n_frames * 320 + emitted * 60
        print(json.dumps({"metric": "ETSI AFE feature frames/sec (NoiseSup + WaveProc + CompCeps + PostProc + VAD)",
                          "value": emitted / (w1 + w2), "unit": "feature frames/s", "ms_per_step": (w1 + w2) * 1e3,
                          "config": {"workload": f"SURVEY 8(f) #3: {n} utterances, {emitted} emitted feature frames of 15 floats",
                                     "ns_with_flags_ms": k1 * 1e3, "waveproc_compceps_postproc_vad_ms": k2 * 1e3},
                          "roofline": {"bound": "hbm", "kernels": "sea::ns_denoise_pipe_fd_kernel + sea::afe_ceps_kernel + sea::afe_vad_kernel",
                                       "achieved": alg / (k1 + k2) / 1e9, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                                       "frac": alg / (k1 + k2) / 1e9 / HBM_PEAK_GBPS, "algorithmic_bytes_per_step": alg,
                                       "avg_step_ms": (k1 + k2) * 1e3}}), flush=True)

    if "host" in what:
        # the host-buffer drop-in path: pack + hipMalloc + H2D + one launch + D2H (PCIe inclusive)
        import ctypes
        lib = sea.load()
        host = batch.data.cpu().numpy()
        ins = [np.ascontiguousarray(host[o:o + l]) for o, l in zip(batch.host_offsets, batch.host_lengths)]
        outs = [np.zeros_like(x) for x in ins]
        n = len(ins)
        pin = (ctypes.c_void_p * n)(*[x.ctypes.data for x in ins])
        pout = (ctypes.c_void_p * n)(*[x.ctypes.data for x in outs])
        lens = (ctypes.c_long * n)(*[x.size for x in ins])
        lib.sea_denoise_utterances(pin, pout, lens, n)
        per = []
        t0 = time.perf_counter()
        for _ in range(args.steps):
            ta = time.perf_counter()
            assert lib.sea_denoise_utterances(pin, pout, lens, n) == 0
            per.append((time.perf_counter() - ta) * 1e3)
        wall = (time.perf_counter() - t0) / args.steps
        # the reference's own calling pattern: one etsi_denoise(short*, short*, long) per utterance
        k = min(n, 128)
        fr1 = int(sum(x.size // 80 for x in ins[:k]))
        lib.etsi_denoise(ins[0].ctypes.data, outs[0].ctypes.data, ins[0].size)
        t1 = time.perf_counter()
        for x, y in zip(ins[:k], outs[:k]):
            assert lib.etsi_denoise(x.ctypes.data, y.ctypes.data, x.size) == 0
        per_call = (time.perf_counter() - t1) / k
        print(json.dumps({"metric": "etsi_denoise() drop-in, one call per utterance (PCIe inclusive)",
                          "value": fr1 / (per_call * k), "unit": "frames/s", "ms_per_step": per_call * 1e3,
                          "config": {"workload": f"{k} sequential calls, mean utterance {fr1 / k:.0f} frames; ms_per_step = per call"}}),
              flush=True)
        print(json.dumps({"metric": "NoiseSup frames/sec through the HOST-buffer entry point (PCIe inclusive)",
                          "value": batch.n_frames / wall, "unit": "frames/s", "ms_per_step": wall * 1e3,
                          "config": {"workload": f"sea_denoise_utterances on {n} host utterances: pack | H2D | launch | D2H | unpack "
                                                 f"pipeline over time slices, {lib.sea_host_threads()} packing threads",
                                     "ms_per_call_sorted": [round(v, 2) for v in sorted(per)]}}), flush=True)

    if "hostrs" in what:
        # resynth() through the host-buffer entry point (PCIe inclusive): int16 + mask rows in, int16 out
        import ctypes
        lib = sea.load()
        host = batch.data.cpu().numpy()
        ins = [np.ascontiguousarray(host[o:o + l]) for o, l in zip(batch.host_offsets, batch.host_lengths)]
        outs = [np.zeros_like(x) for x in ins]
        rng = np.random.default_rng(5)
        masks = [rng.random(((x.size - 320) // 160 + 1, 64), dtype=np.float32) for x in ins]
        n = len(ins)
        pin = (ctypes.c_void_p * n)(*[x.ctypes.data for x in ins])
        pm = (ctypes.c_void_p * n)(*[m.ctypes.data for m in masks])
        pout = (ctypes.c_void_p * n)(*[x.ctypes.data for x in outs])
        lens = (ctypes.c_long * n)(*[x.size for x in ins])
        hops = int(sum(m.shape[0] for m in masks))
        for binary in (0, 1):
            assert lib.sea_resynth_utterances(pin, lens, pm, binary, pout, n) == 0, lib.sea_last_error()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                assert lib.sea_resynth_utterances(pin, lens, pm, binary, pout, n) == 0
            wall = (time.perf_counter() - t0) / args.steps
            print(json.dumps({"metric": f"resynth hop-frames/sec through the HOST-buffer entry point (PCIe inclusive), {'IBM' if binary else 'ratio mask'}",
                              "value": hops / wall, "unit": "hop-frames/s", "ms_per_step": wall * 1e3,
                              "config": {"workload": f"sea_resynth_utterances on {n} host utterances, {hops} mask rows"}}), flush=True)

    if "wb" in what:
        # the ETSI wideband (16 kHz) mode: the corpus plus as many wideband signals of the same lengths (the corpus alone
        # never moves the high band's VAD), QMF + low-band NoiseSup + high band, then the 26-band CompCeps; device events,
        # warm-up discarded, MEDIAN of the steps
        lib = sea.load()
        wb = wb_batch(batch, dev)
        n, total = wb.n_utt, wb.total
        half = (total // 2 + 7) // 8 * 8
        out = torch.zeros(half, dtype=torch.int16, device=dev)
        f32 = torch.zeros(half, dtype=torch.float32, device=dev)
        first = torch.full((n,), -1, dtype=torch.int32, device=dev)
        onset = torch.zeros(n, dtype=torch.int32, device=dev)
        rows = int(lib.sea_wb_rows(total))
        hpr = torch.zeros((rows, 3), dtype=torch.float32, device=dev)
        code = torch.zeros((rows, 9), dtype=torch.float32, device=dev)
        scratch = torch.zeros(int(lib.sea_wb_scratch_bytes(total, n)) // 4 + 4, dtype=torch.float32, device=dev)
        cap = np.maximum(np.asarray(wb.host_lengths) // 160 - 6, 0).astype(np.int64)
        cum = np.concatenate(([0], np.cumsum(cap))).astype(np.int64)
        tc = int(cum[-1])
        ceps = torch.zeros((max(tc, 1), 14), dtype=torch.float32, device=dev)
        ncep = torch.zeros(n, dtype=torch.int32, device=dev)
        d_cum = torch.from_numpy(cum).to(dev)
        P = lambda t: t.data_ptr()
        st = torch.cuda.current_stream().cuda_stream

        def denoise():
            assert lib.sea_wb_denoise_batch(P(wb.data), P(out), P(f32), P(wb.offsets), P(wb.lengths), P(wb.order), P(first),
                                            P(onset), P(hpr), P(code), P(scratch), total, n, st) == 0, lib.sea_last_error()

        def cepstra():
            assert lib.sea_wb_compceps_batch(P(f32), P(wb.offsets), P(wb.lengths), P(first), P(hpr), P(code), P(d_cum), tc,
                                             P(ceps), P(ncep), n, st) == 0, lib.sea_last_error()
        steps = max(args.steps, 5)
        m1, t1 = median_ms(denoise, steps)
        m2, t2 = median_ms(cepstra, steps)
        frames = int(np.sum(np.asarray(wb.host_lengths) // 160))
        print(json.dumps({"metric": "ETSI wideband mode frames/sec (160-sample frames: QMF + low-band NoiseSup + high band + 26-band CompCeps)",
                          "value": frames / ((m1 + m2) / 1e3), "unit": "frames/s", "ms_per_step": m1 + m2,
                          "config": {"workload": f"{n} utterances at 16 kHz: the {args.utts}-utterance corpus + as many wideband signals of "
                                                 f"the same lengths, {frames} frames, {int(ncep.sum().item())} cepstral frames; median of {steps}",
                                     "wb_denoise_batch_ms": m1, "wb_compceps_batch_ms": m2,
                                     "wb_denoise_batch_ms_sorted": [round(v, 3) for v in t1],
                                     "wb_compceps_batch_ms_sorted": [round(v, 3) for v in t2]},
                          "kernels": "sea::wb_qmf_kernel + sea::ns_denoise_pipe_wb_kernel + sea::wb_hb_kernel + sea::wb_specsub_kernel + "
                                     "sea::compceps_wb_kernel",
                          "algorithmic_bytes_per_frame": {"wb_qmf_kernel": 160 * 2 + 2 * 80 * 4, "wb_hb_kernel": 2 * 80 * 4 + 12 * 4}}),
              flush=True)

    if "wbafe" in what:
        # the wideband mode's FEATURE CHAIN on the batch of --what wb, one line per launch group and one for the whole path:
        # QMF + low-band NoiseSup with speech flags + high band | WaveProc + 26-band CompCeps | PostProc + VAD + flush; device
        # events, warm-up discarded, MEDIAN of the steps.  The library launches the last two groups from one call: the third is
        # timed alone (total_ceps = 0 skips the second, the cepstra of the run before stay in place), the second is the whole
        # call's median minus the third's
        lib = sea.load()
        wb = wb_batch(batch, dev)
        n, total = wb.n_utt, wb.total
        half = (total // 2 + 7) // 8 * 8
        out = torch.zeros(half, dtype=torch.int16, device=dev)
        f32 = torch.zeros(half, dtype=torch.float32, device=dev)
        first = torch.full((n,), -1, dtype=torch.int32, device=dev)
        onset = torch.zeros(n, dtype=torch.int32, device=dev)
        rows = int(lib.sea_wb_rows(total))
        flg = torch.zeros(rows, dtype=torch.uint8, device=dev)
        hpr = torch.zeros((rows, 3), dtype=torch.float32, device=dev)
        code = torch.zeros((rows, 9), dtype=torch.float32, device=dev)
        scratch = torch.zeros(int(lib.sea_wb_scratch_bytes(total, n)) // 4 + 4, dtype=torch.float32, device=dev)
        nfr = np.asarray(wb.host_lengths) // 160
        ccum = np.concatenate(([0], np.cumsum(np.maximum(nfr - 6, 0)))).astype(np.int64)
        fcum = np.concatenate(([0], np.cumsum(nfr + 6))).astype(np.int64)
        tc, tf = int(ccum[-1]), int(fcum[-1])
        fcc = torch.zeros((max(tc, 1), 14), dtype=torch.float32, device=dev)
        f15 = torch.zeros((max(tf, 1), 15), dtype=torch.float32, device=dev)
        nfe = torch.zeros(n, dtype=torch.int32, device=dev)
        ncep = torch.zeros(n, dtype=torch.int32, device=dev)
        d_ccum, d_fcum = torch.from_numpy(ccum).to(dev), torch.from_numpy(fcum).to(dev)
        P = lambda t: t.data_ptr()
        st = torch.cuda.current_stream().cuda_stream

        def denoise_fd():
            assert lib.sea_wb_denoise_batch_fd(P(wb.data), P(out), P(f32), P(wb.offsets), P(wb.lengths), P(wb.order), P(first),
                                               P(onset), P(flg), P(hpr), P(code), P(scratch), total, n, st) == 0, lib.sea_last_error()

        def features(total_ceps):
            assert lib.sea_wb_afe_features_batch(P(f32), P(flg), P(hpr), P(code), P(wb.offsets), P(wb.lengths), P(first), P(onset),
                                                 P(d_ccum), total_ceps, P(fcc), None, P(d_fcum), P(f15), P(nfe), P(ncep), n,
                                                 st) == 0, lib.sea_last_error()
        steps = max(args.steps, 5)
        m1, t1 = median_ms(denoise_fd, steps)
        m23, t23 = median_ms(lambda: features(tc), steps)
        m3, t3 = median_ms(lambda: features(0), steps)
        m2 = m23 - m3
        frames, emitted = int(nfr.sum()), int(nfe.sum().item())
        workload = (f"{n} utterances at 16 kHz: the {args.utts}-utterance corpus + as many wideband signals of the same lengths, "
                    f"{frames} frames, {int(ncep.sum().item())} cepstral frames, {emitted} emitted feature frames; median of {steps}")
        for group, ms, kernels, extra in (
                ("QMF + low-band NoiseSup with speech flags + high band", m1,
                 "sea::wb_qmf_kernel + sea::ns_denoise_pipe_wb_fd_kernel + sea::wb_hb_kernel + sea::wb_specsub_kernel",
                 {"ms_sorted": [round(v, 3) for v in t1]}),
                ("WaveProc + 26-band CompCeps", m2, "sea::afe_wb_ceps_kernel",
                 {"derived": "median of the features call minus the median of its PostProc + VAD launch alone",
                  "features_call_ms_sorted": [round(v, 3) for v in t23]}),
                ("PostProc + VAD + flush", m3, "sea::afe_wb_vad_kernel", {"ms_sorted": [round(v, 3) for v in t3]})):
            print(json.dumps({"metric": f"ETSI wideband feature chain, launch group: {group} (frames of 160 samples/sec)",
                              "value": frames / (ms / 1e3), "unit": "frames/s", "ms_per_step": ms,
                              "config": dict(workload=workload, **extra), "kernels": kernels}), flush=True)
        print(json.dumps({"metric": "ETSI wideband feature chain frames/sec (160-sample frames: QMF + NoiseSup with flags + high band "
                                    "+ WaveProc + 26-band CompCeps + PostProc + VAD)",
                          "value": frames / ((m1 + m23) / 1e3), "unit": "frames/s", "ms_per_step": m1 + m23,
                          "config": {"workload": workload, "wb_denoise_batch_fd_ms": m1, "waveproc_compceps_ms": m2,
                                     "postproc_vad_ms": m3, "wb_afe_features_batch_ms": m23}}), flush=True)

    if "wbslices" in what:
        # The wideband mode cut along the TIME axis, on the batch of --what wb.  Three lines:
        #   (i)   sea_wb_denoise_batch, the one launch: the yardstick
        #   (ii)  the same batch as 4 and as 8 slices of equal frame shares, one sea_wb_denoise_batch_slice per slice, device only
        #         (every slice's packed input is resident before the clock starts)
        #   (iii) sea_wb_denoise_utterances from pageable host arrays, wall clock around calls that return with the results
        #         on the host: PCIe inclusive
        # (i) and (ii): device events around every step, one warm-up step of every shape discarded, the steps of the three
        # forms ALTERNATING in one loop, median and the sorted list of each.  All in frames of 160 samples per second.
        import ctypes
        lib = sea.load()
        wb = wb_batch(batch, dev)
        n, total = wb.n_utt, wb.total
        lens = np.asarray(wb.host_lengths)
        nfr = lens // 160
        frames = int(nfr.sum())
        host = wb.data.cpu().numpy()
        utts = [host[o:o + l] for o, l in zip(wb.host_offsets, lens)]
        P = lambda t: t.data_ptr() if t is not None else None
        st = torch.cuda.current_stream().cuda_stream

        class Bufs:  # the outputs and the scratch of one launch over a PackedBatch
            def __init__(self, b):
                half = (b.total // 2 + 7) // 8 * 8
                rows = int(lib.sea_wb_rows(b.total))
                self.b = b
                self.out = torch.zeros(half, dtype=torch.int16, device=dev)
                self.hpr = torch.zeros((rows, 3), dtype=torch.float32, device=dev)
                self.code = torch.zeros((rows, 9), dtype=torch.float32, device=dev)
                self.scratch = torch.zeros(int(lib.sea_wb_scratch_bytes(b.total, b.n_utt)) // 4 + 4, dtype=torch.float32, device=dev)
        whole = Bufs(wb)
        first = torch.full((n,), -1, dtype=torch.int32, device=dev)
        onset = torch.zeros(n, dtype=torch.int32, device=dev)

        def one_launch():
            assert lib.sea_wb_denoise_batch(P(wb.data), P(whole.out), None, P(wb.offsets), P(wb.lengths), P(wb.order), P(first),
                                            P(onset), P(whole.hpr), P(whole.code), P(whole.scratch), total, n, st) == 0, lib.sea_last_error()
        idx = np.argsort(-nfr, kind="stable")
        snfr = nfr[idx]
        state = torch.zeros((n, int(lib.sea_wb_slice_state_floats())), dtype=torch.float32, device=dev)
        sfirst, sonset = torch.full_like(first, -1), torch.zeros_like(onset)

        def cut(nslices):  # boundaries with equal shares of the frames, as the host pipeline cuts
            bounds = [0]
            for k in range(1, nslices):
                share = frames * k // nslices
                f = next(f for f in range(bounds[-1] + 1, int(snfr[0]) + 1) if int(np.minimum(snfr, f).sum()) >= share)
                if f >= snfr[0]:
                    break
                bounds.append(f)
            bounds.append(int(snfr[0]))
            pieces = []
            for b0, b1 in zip(bounds[:-1], bounds[1:]):
                act = [int(u) for u in idx[snfr > b0]]
                pieces.append((b0, Bufs(sea.PackedBatch.from_arrays([utts[u][160 * b0:160 * min(b1, int(nfr[u]))] for u in act], dev))))
            return pieces

        def run_slices(pieces):
            for k, (b0, B) in enumerate(pieces):
                b = B.b
                assert lib.sea_wb_denoise_batch_slice(P(b.data), P(B.out), None, P(b.offsets), P(b.lengths), P(b.order), P(sfirst),
                                                      P(sonset), P(B.hpr), P(B.code), P(B.scratch), b.total, P(state), b.n_utt, b0,
                                                      1 if k else 0, st) == 0, lib.sea_last_error()
        forms = [("one launch", one_launch)] + [(f"{len(p)} slices", (lambda p=p: run_slices(p))) for p in (cut(4), cut(8))]
        steps = max(args.steps, 5)
        for _, fn in forms:
            fn()
        torch.cuda.synchronize()
        ev = {name: [] for name, _ in forms}
        for _ in range(steps):
            for name, fn in forms:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                ev[name].append((a, b))
        torch.cuda.synchronize()
        # the sliced runs saw the utterances longest first: the same indices, permuted
        assert torch.equal(sfirst.cpu(), first.cpu()[torch.from_numpy(idx)]) and torch.equal(sonset.cpu(), onset.cpu()[torch.from_numpy(idx)])
        med = {}
        for name, _ in forms:
            t = sorted(a.elapsed_time(b) for a, b in ev[name])
            med[name] = t[len(t) // 2]
            print(json.dumps({"metric": f"ETSI wideband mode, QMF + low-band NoiseSup + high band, {name}, device only (frames of 160 samples/sec)",
                              "value": frames / (med[name] / 1e3), "unit": "frames/s", "ms_per_step": med[name],
                              "config": {"workload": f"{n} utterances at 16 kHz: the {args.utts}-utterance corpus + as many wideband signals of "
                                                     f"the same lengths, {frames} frames; median of {steps} alternating steps",
                                         "ms_sorted": [round(v, 3) for v in t],
                                         "ratio_to_one_launch": round(med[name] / med["one launch"], 3)},
                              "kernels": "sea::wb_qmf_kernel + sea::ns_denoise_pipe_wb_kernel + sea::wb_hb_kernel + sea::wb_specsub_kernel"
                                         if name == "one launch" else
                                         "per slice: sea::wb_qmf_slice_kernel + sea::ns_denoise_pipe_wb_slice_kernel + sea::wb_hb_slice_kernel + "
                                         "sea::wb_slice_end_kernel"}), flush=True)
        del forms, whole
        outs = [np.zeros(int(f) * 80, np.int16) for f in nfr]
        hps = [np.zeros((int(f), 3), np.float32) for f in nfr]
        codes = [np.zeros((int(f), 9), np.float32) for f in nfr]
        ptr = lambda arrs: (ctypes.c_void_p * n)(*[x.ctypes.data for x in arrs])
        pin, pout, php, pcode = ptr(utts), ptr(outs), ptr(hps), ptr(codes)
        plen = (ctypes.c_long * n)(*[int(l) for l in lens])
        res = {}
        for name, a, b in (("low band only", None, None), ("low band + high-band rows", php, pcode)):
            assert lib.sea_wb_denoise_utterances(pin, pout, a, b, plen, n) == 0, lib.sea_last_error()
            t = []
            for _ in range(steps):
                t0 = time.perf_counter()
                assert lib.sea_wb_denoise_utterances(pin, pout, a, b, plen, n) == 0, lib.sea_last_error()
                t.append((time.perf_counter() - t0) * 1e3)
            t.sort()
            res[name] = (t[len(t) // 2], [round(v, 3) for v in t])
        m = res["low band only"][0]
        print(json.dumps({"metric": "ETSI wideband mode through the HOST-buffer pipeline sea_wb_denoise_utterances (PCIe inclusive, frames of 160 samples/sec)",
                          "value": frames / (m / 1e3), "unit": "frames/s", "ms_per_step": m,
                          "config": {"workload": f"{n} host utterances at 16 kHz, {frames} frames, {int(lib.sea_host_last_slices())} slices, "
                                                 f"{lib.sea_host_threads()} packing threads; wall clock, median of {steps} calls after one warm-up",
                                     "ms_sorted": res["low band only"][1],
                                     "with_high_band_rows_ms": res["low band + high-band rows"][0],
                                     "with_high_band_rows_ms_sorted": res["low band + high-band rows"][1]}}), flush=True)

    if "wbafeslices" in what:
        # The wideband FEATURE CHAIN cut along the TIME axis, on the batch of --what wbafe.  Side by side:
        #   (i)   sea_wb_denoise_batch_fd + sea_wb_afe_features_batch, the one launch group: the yardstick
        #   (ii)  the same batch as 8 slices of equal frame shares, sea_wb_denoise_batch_slice_fd +
        #         sea_wb_afe_features_batch_slice per slice, device only (every slice's packed input is resident)
        #   (iii) the same chain on ONE slice of one frame per utterance: the fixed cost of a slice's launches
        #   (iv)  sea_wb_features_utterances from pageable host arrays, wall clock, PCIe inclusive
        # (i)-(iii): device events around every step, one warm-up step of every form discarded, the steps of the forms
        # ALTERNATING in one loop, median and the sorted list of each.
        import ctypes
        lib = sea.load()
        wb = wb_batch(batch, dev)
        n = wb.n_utt
        lens = np.asarray(wb.host_lengths)
        nfr = lens // 160
        frames = int(nfr.sum())
        host = wb.data.cpu().numpy()
        utts = [host[o:o + l] for o, l in zip(wb.host_offsets, lens)]
        P = lambda t: t.data_ptr() if t is not None else None
        st = torch.cuda.current_stream().cuda_stream

        class Chain:  # everything one launch group over a PackedBatch reads and writes; ccap / fcap: rows per utterance of feat_cc / feat15
            def __init__(self, b, ccap, fcap, final=None):
                half = (b.total // 2 + 7) // 8 * 8
                rows = int(lib.sea_wb_rows(b.total))
                z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
                self.b = b
                self.out, self.f32 = z(half, torch.int16), z(half, torch.float32)
                self.flg, self.hpr, self.code = z(rows, torch.uint8), z((rows, 3), torch.float32), z((rows, 9), torch.float32)
                self.scratch = z(int(lib.sea_wb_scratch_bytes(b.total, b.n_utt)) // 4 + 4, torch.float32)
                ccum = np.concatenate(([0], np.cumsum(ccap))).astype(np.int64)
                fcum = np.concatenate(([0], np.cumsum(fcap))).astype(np.int64)
                self.tc = int(ccum[-1])
                self.fcc, self.f15 = z((max(self.tc, 1), 14), torch.float32), z((max(int(fcum[-1]), 1), 15), torch.float32)
                self.nfe, self.ncep = z(b.n_utt, torch.int32), z(b.n_utt, torch.int32)
                self.ccum, self.fcum = torch.from_numpy(ccum).to(dev), torch.from_numpy(fcum).to(dev)
                self.final = torch.from_numpy(np.asarray(final, np.uint8)).to(dev) if final is not None else None
        whole = Chain(wb, np.maximum(nfr - 6, 0), nfr + 6)
        first = torch.full((n,), -1, dtype=torch.int32, device=dev)
        onset = torch.zeros(n, dtype=torch.int32, device=dev)

        def one_launch(denoise=True, features=True):
            C, b = whole, wb
            if denoise:
                rc = lib.sea_wb_denoise_batch_fd(P(b.data), P(C.out), P(C.f32), P(b.offsets), P(b.lengths), P(b.order), P(first), P(onset),
                                                 P(C.flg), P(C.hpr), P(C.code), P(C.scratch), b.total, n, st)
                assert rc == 0, lib.sea_last_error()
            if features:
                rc = lib.sea_wb_afe_features_batch(P(C.f32), P(C.flg), P(C.hpr), P(C.code), P(b.offsets), P(b.lengths), P(first), P(onset),
                                                   P(C.ccum), C.tc, P(C.fcc), None, P(C.fcum), P(C.f15), P(C.nfe), P(C.ncep), n, st)
                assert rc == 0, lib.sea_last_error()
        idx = np.argsort(-nfr, kind="stable")
        snfr = nfr[idx]
        state = torch.zeros((n, int(lib.sea_wb_slice_state_floats())), dtype=torch.float32, device=dev)
        afe = torch.zeros((n, int(lib.sea_wb_afe_slice_state_floats())), dtype=torch.float32, device=dev)
        sfirst, sonset = torch.full_like(first, -1), torch.zeros_like(onset)

        def cut(bounds):
            pieces = []
            for b0, b1 in zip(bounds[:-1], bounds[1:]):
                act = [int(u) for u in idx[snfr > b0]]
                fr = np.array([min(b1, int(nfr[u])) - b0 for u in act], np.int64)
                pb = sea.PackedBatch.from_arrays([utts[u][160 * b0:160 * min(b1, int(nfr[u]))] for u in act], dev)
                pieces.append((b0, Chain(pb, fr, fr + 6, [int(nfr[u]) <= b1 for u in act])))
            return pieces

        def equal_shares(nslices):  # boundaries with equal shares of the frames, as the host pipeline cuts
            bounds = [0]
            for k in range(1, nslices):
                share = frames * k // nslices
                f = next(f for f in range(bounds[-1] + 1, int(snfr[0]) + 1) if int(np.minimum(snfr, f).sum()) >= share)
                if f >= snfr[0]:
                    break
                bounds.append(f)
            return bounds + [int(snfr[0])]

        def run_slices(pieces, denoise=True, features=True):
            for k, (b0, C) in enumerate(pieces):
                b = C.b
                if denoise:
                    rc = lib.sea_wb_denoise_batch_slice_fd(P(b.data), P(C.out), P(C.f32), P(b.offsets), P(b.lengths), P(b.order),
                                                           P(sfirst), P(sonset), P(C.flg), P(C.hpr), P(C.code), P(C.scratch), b.total,
                                                           P(state), b.n_utt, b0, 1 if k else 0, st)
                    assert rc == 0, lib.sea_last_error()
                if features:
                    rc = lib.sea_wb_afe_features_batch_slice(P(C.f32), P(C.flg), P(C.hpr), P(C.code), P(b.offsets), P(b.lengths),
                                                             P(sfirst), P(sonset), P(C.final), P(C.ccum), C.tc, P(C.fcc), None,
                                                             P(C.fcum), P(C.f15), P(C.nfe), P(C.ncep), P(afe), b.n_utt, b0,
                                                             1 if k else 0, st)
                    assert rc == 0, lib.sea_last_error()
        p8 = cut(equal_shares(8))
        p1 = cut([0, 1])[:1]
        for _, C in p1:
            C.final = None  # one frame of every utterance, nothing ends: the launches' fixed cost
        forms = [("one launch group", one_launch), (f"{len(p8)} slices", lambda: run_slices(p8)),
                 ("one slice of one frame per utterance", lambda: run_slices(p1)),
                 # each step alone, on what the whole chain left in place: which of the two accounts for the slices' cost
                 ("one launch group, step 1 alone", lambda: one_launch(features=False)),
                 ("one launch group, step 2 alone", lambda: one_launch(denoise=False)),
                 ("slices, step 1 alone", lambda: run_slices(p8, features=False)),
                 ("slices, step 2 alone", lambda: run_slices(p8, denoise=False))]
        steps = max(args.steps, 7)
        for _, fn in forms:
            fn()
        torch.cuda.synchronize()
        ev = {name: [] for name, _ in forms}
        for _ in range(steps):
            for name, fn in forms:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                ev[name].append((a, b))
        torch.cuda.synchronize()
        run_slices(p8)  # once more after the one-frame form, for the comparison of the counts below
        torch.cuda.synchronize()
        emitted = int(whole.nfe.sum().item())
        assert sum(int(C.nfe.sum().item()) for _, C in p8) == emitted, "the slices' emitted frames do not sum to the one launch's"
        med, srt = {}, {}
        for name, _ in forms:
            t = sorted(a.elapsed_time(b) for a, b in ev[name])
            med[name], srt[name] = t[len(t) // 2], [round(v, 3) for v in t]
        outs = [np.zeros(int(f) * 80, np.int16) for f in nfr]
        feats = [np.zeros((int(f) + 6, 15), np.float32) for f in nfr]
        ptr = lambda arrs: (ctypes.c_void_p * n)(*[x.ctypes.data for x in arrs])
        pin, pout, pfeat = ptr(utts), ptr(outs), ptr(feats)
        plen = (ctypes.c_long * n)(*[int(l) for l in lens])
        pnf = (ctypes.c_int * n)()
        hostres = {}
        for name, po in (("features only", None), ("features + low band", pout)):
            rc = lib.sea_wb_features_utterances(pin, po, pfeat, pnf, plen, n)
            assert rc == 0, lib.sea_last_error()
            t = []
            for _ in range(steps):
                t0 = time.perf_counter()
                rc = lib.sea_wb_features_utterances(pin, po, pfeat, pnf, plen, n)
                t.append((time.perf_counter() - t0) * 1e3)
                assert rc == 0, lib.sea_last_error()
            t.sort()
            hostres[name] = (t[len(t) // 2], [round(v, 3) for v in t])
        assert sum(pnf) == emitted, "the host pipeline's emitted frames are not the one launch's"
        k8, one, fix = f"{len(p8)} slices", med["one launch group"], med["one slice of one frame per utterance"]
        print(json.dumps({
            "metric": "ETSI wideband feature chain in time slices: one launch group | slices | host pipeline (frames of 160 samples/sec)",
            "value": frames / (med[k8] / 1e3), "unit": "frames/s", "ms_per_step": med[k8],
            "config": {"workload": f"{n} utterances at 16 kHz: the {args.utts}-utterance corpus + as many wideband signals of the same "
                                   f"lengths, {frames} frames, {emitted} emitted feature frames; device forms: median of {steps} "
                                   f"alternating steps after one warm-up; host pipeline: wall clock, median of {steps} calls",
                       "slices": len(p8), "one_launch_group_ms": one, "one_launch_group_ms_sorted": srt["one launch group"],
                       "slices_ms": med[k8], "slices_ms_sorted": srt[k8], "ratio_to_one_launch_group": round(med[k8] / one, 3),
                       "one_frame_slice_ms": fix, "one_frame_slice_ms_sorted": srt["one slice of one frame per utterance"],
                       "slices_minus_one_launch_ms": round(med[k8] - one, 3), "fixed_cost_of_the_slices_ms": round(len(p8) * fix, 3),
                       "step1_alone_ms": {"one_launch_group": med["one launch group, step 1 alone"], "slices": med["slices, step 1 alone"],
                                          "one_launch_group_sorted": srt["one launch group, step 1 alone"], "slices_sorted": srt["slices, step 1 alone"]},
                       "step2_alone_ms": {"one_launch_group": med["one launch group, step 2 alone"], "slices": med["slices, step 2 alone"],
                                          "one_launch_group_sorted": srt["one launch group, step 2 alone"], "slices_sorted": srt["slices, step 2 alone"]},
                       "host_pipeline_ms": hostres["features only"][0], "host_pipeline_ms_sorted": hostres["features only"][1],
                       "host_pipeline_slices": int(lib.sea_host_last_slices()), "host_threads": lib.sea_host_threads(),
                       "host_pipeline_with_low_band_ms": hostres["features + low band"][0],
                       "host_pipeline_with_low_band_ms_sorted": hostres["features + low band"][1]},
            "kernels": "per slice: sea::wb_qmf_slice_kernel + sea::ns_denoise_pipe_wb_fd_slice_kernel + sea::wb_hb_slice_kernel + "
                       "sea::wb_slice_end_kernel + sea::afe_wb_ceps_slice_kernel + sea::afe_wb_vad_slice_kernel"}), flush=True)

    if "afeslices" in what:
        # The 8 kHz FEATURE CHAIN cut along the TIME axis, on the --utts corpus batch.  Side by side in one process:
        #   (i)   sea_ns_denoise_batch_fd + sea_afe_features_batch, the one launch group: the baseline to quote against
        #   (ii)  the same batch as 8 slices of equal frame shares, sea_ns_denoise_batch_slice_fd + sea_afe_features_batch_slice
        #         per slice, device only (every slice's packed input is resident)
        #   (iii) sea_features_utterances from pageable host arrays, wall clock, PCIe inclusive
        # (i), (ii): device events around every step, one warm-up step of either form discarded, the steps of the forms
        # ALTERNATING in one loop, median and the sorted list of each.
        import ctypes
        lib = sea.load()
        n = batch.n_utt
        lens = np.asarray(batch.host_lengths)
        nfr = lens // 80
        frames = int(nfr.sum())
        host = batch.data.cpu().numpy()
        utts = [host[o:o + l] for o, l in zip(batch.host_offsets, lens)]
        P = lambda t: t.data_ptr() if t is not None else None
        st = torch.cuda.current_stream().cuda_stream

        class Chain:  # everything one launch group over a PackedBatch reads and writes; ccap / fcap: rows per utterance of feat_cc / feat15
            def __init__(self, b, ccap, fcap, final=None):
                z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
                self.b = b
                self.out, self.f32 = torch.zeros_like(b.data), z(b.data.numel(), torch.float32)
                self.flg = z(max(b.total // 8, 1), torch.uint8)
                ccum = np.concatenate(([0], np.cumsum(ccap))).astype(np.int64)
                fcum = np.concatenate(([0], np.cumsum(fcap))).astype(np.int64)
                self.tc = int(ccum[-1])
                self.fcc, self.f15 = z((max(self.tc, 1), 14), torch.float32), z((max(int(fcum[-1]), 1), 15), torch.float32)
                self.nfe, self.ncep = z(b.n_utt, torch.int32), z(b.n_utt, torch.int32)
                self.ccum, self.fcum = torch.from_numpy(ccum).to(dev), torch.from_numpy(fcum).to(dev)
                self.final = torch.from_numpy(np.asarray(final, np.uint8)).to(dev) if final is not None else None
        whole = Chain(batch, np.maximum(nfr - 6, 0), nfr + 6)
        first = torch.full((n,), -1, dtype=torch.int32, device=dev)
        onset = torch.zeros(n, dtype=torch.int32, device=dev)

        def one_launch(denoise=True, features=True):
            C, b = whole, batch
            if denoise:
                rc = lib.sea_ns_denoise_batch_fd(P(b.data), P(C.out), P(C.f32), P(b.offsets), P(b.lengths), P(b.order), P(first),
                                                 P(C.flg), P(onset), n, st)
                assert rc == 0, lib.sea_last_error()
            if features:
                rc = lib.sea_afe_features_batch(P(C.f32), P(C.flg), P(b.offsets), P(b.lengths), P(first), P(onset), P(C.ccum), C.tc,
                                                P(C.fcc), None, P(C.fcum), P(C.f15), P(C.nfe), P(C.ncep), n, st)
                assert rc == 0, lib.sea_last_error()
        idx = np.argsort(-nfr, kind="stable")
        snfr = nfr[idx]
        state = torch.zeros((n, int(lib.sea_ns_slice_state_floats())), dtype=torch.float32, device=dev)
        afe = torch.zeros((n, int(lib.sea_afe_slice_state_floats())), dtype=torch.float32, device=dev)
        sfirst, sonset = torch.full_like(first, -1), torch.zeros_like(onset)
        bounds = [0]
        for k in range(1, 8):  # boundaries with equal shares of the frames, as the host pipeline cuts
            share = frames * k // 8
            f = next(f for f in range(bounds[-1] + 1, int(snfr[0]) + 1) if int(np.minimum(snfr, f).sum()) >= share)
            if f >= snfr[0]:
                break
            bounds.append(f)
        bounds.append(int(snfr[0]))
        pieces = []
        for b0, b1 in zip(bounds[:-1], bounds[1:]):
            act = [int(u) for u in idx[snfr > b0]]
            fr = np.array([min(b1, int(nfr[u])) - b0 for u in act], np.int64)
            pb = sea.PackedBatch.from_arrays([utts[u][80 * b0:80 * min(b1, int(nfr[u]))] for u in act], dev)
            pieces.append((b0, Chain(pb, fr, fr + 6, [int(nfr[u]) <= b1 for u in act])))

        def run_slices(denoise=True, features=True):
            for k, (b0, C) in enumerate(pieces):
                b = C.b
                if denoise:
                    rc = lib.sea_ns_denoise_batch_slice_fd(P(b.data), P(C.out), P(C.f32), P(b.offsets), P(b.lengths), P(b.order),
                                                           P(sfirst), P(C.flg), P(sonset), P(state), b.n_utt, b0, 1 if k else 0, st)
                    assert rc == 0, lib.sea_last_error()
                if features:
                    rc = lib.sea_afe_features_batch_slice(P(C.f32), P(C.flg), P(b.offsets), P(b.lengths), P(sfirst), P(sonset),
                                                          P(C.final), P(C.ccum), C.tc, P(C.fcc), None, P(C.fcum), P(C.f15), P(C.nfe),
                                                          P(C.ncep), P(afe), b.n_utt, b0, 1 if k else 0, st)
                    assert rc == 0, lib.sea_last_error()
        k8 = f"{len(pieces)} slices"
        forms = [("one launch group", one_launch), (k8, run_slices),
                 # each step alone, on what the whole chain left in place: which of the two accounts for the slices' cost
                 ("one launch group, step 1 alone", lambda: one_launch(features=False)),
                 ("one launch group, step 2 alone", lambda: one_launch(denoise=False)),
                 ("slices, step 1 alone", lambda: run_slices(features=False)),
                 ("slices, step 2 alone", lambda: run_slices(denoise=False))]
        steps = max(args.steps, 7)
        for _, fn in forms:
            fn()
        torch.cuda.synchronize()
        ev = {name: [] for name, _ in forms}
        for _ in range(steps):
            for name, fn in forms:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                ev[name].append((a, b))
        torch.cuda.synchronize()
        run_slices()  # the whole chain once more after the steps alone, for the comparison of the counts below
        torch.cuda.synchronize()
        emitted = int(whole.nfe.sum().item())
        assert sum(int(C.nfe.sum().item()) for _, C in pieces) == emitted, "the slices' emitted frames do not sum to the one launch's"
        med, srt = {}, {}
        for name, _ in forms:
            t = sorted(a.elapsed_time(b) for a, b in ev[name])
            med[name], srt[name] = t[len(t) // 2], [round(v, 3) for v in t]
        feats = [np.zeros((int(f) + 6, 15), np.float32) for f in nfr]
        ptr = lambda arrs: (ctypes.c_void_p * n)(*[x.ctypes.data for x in arrs])
        pin, pfeat = ptr(utts), ptr(feats)
        plen = (ctypes.c_long * n)(*[int(l) for l in lens])
        pnf = (ctypes.c_int * n)()
        rc = lib.sea_features_utterances(pin, None, pfeat, pnf, plen, n)
        assert rc == 0, lib.sea_last_error()
        t = []
        for _ in range(steps):
            t0 = time.perf_counter()
            rc = lib.sea_features_utterances(pin, None, pfeat, pnf, plen, n)
            t.append((time.perf_counter() - t0) * 1e3)
            assert rc == 0, lib.sea_last_error()
        t.sort()
        assert sum(pnf) == emitted, "the host pipeline's emitted frames are not the one launch's"
        one = med["one launch group"]
        print(json.dumps({
            "metric": "8 kHz feature chain in time slices: one launch group | slices | host pipeline (frames of 80 samples/sec)",
            "value": frames / (med[k8] / 1e3), "unit": "frames/s", "ms_per_step": med[k8],
            "config": {"workload": f"the {args.utts}-utterance corpus at 8 kHz, {frames} frames, {emitted} emitted feature frames; device "
                                   f"forms: median of {steps} alternating steps after one warm-up; host pipeline: wall clock, median "
                                   f"of {steps} calls",
                       "slices": len(pieces), "one_launch_group_ms": one, "one_launch_group_ms_sorted": srt["one launch group"],
                       "slices_ms": med[k8], "slices_ms_sorted": srt[k8], "ratio_to_one_launch_group": round(med[k8] / one, 3),
                       "step1_alone_ms": {"one_launch_group": med["one launch group, step 1 alone"], "slices": med["slices, step 1 alone"],
                                          "one_launch_group_sorted": srt["one launch group, step 1 alone"], "slices_sorted": srt["slices, step 1 alone"]},
                       "step2_alone_ms": {"one_launch_group": med["one launch group, step 2 alone"], "slices": med["slices, step 2 alone"],
                                          "one_launch_group_sorted": srt["one launch group, step 2 alone"], "slices_sorted": srt["slices, step 2 alone"]},
                       "host_pipeline_ms": t[len(t) // 2], "host_pipeline_ms_sorted": [round(v, 3) for v in t],
                       "host_pipeline_slices": int(lib.sea_host_last_slices()), "host_threads": lib.sea_host_threads()},
            "kernels": "one launch group: sea::ns_denoise_pipe6_fd_kernel or sea::ns_denoise_pipe_fd_kernel + sea::afe_ceps_kernel + "
                       "sea::afe_vad_kernel; per slice: sea::ns_denoise_pipe_fd_slice_kernel + sea::afe_ceps_slice_kernel + "
                       "sea::afe_vad_slice_kernel"}), flush=True)

    if "cepsslices" in what:
        # NoiseSup + the plain CompCeps (no WaveProc) cut along the TIME axis, at 8 kHz on the --utts corpus batch (--what afeslices')
        # and in the wideband mode on the batch of --what wbafeslices.  Side by side in one process, per rate:
        #   (i)   the one launch group: sea_ns_denoise_batch + sea_compceps_batch (sea_wb_denoise_batch + sea_wb_compceps_batch)
        #   (ii)  the same batch as 8 slices of equal frame shares, the denoiser's slice call + sea_compceps_batch_slice
        #         (sea_wb_compceps_batch_slice) per slice, device only (every slice's packed input is resident)
        #   (iii) the host call from pageable host arrays, wall clock, PCIe inclusive: sea_denoise_ceps_utterances with
        #         SEA_HOST_CEPS_PIPELINE=0 (one launch each, the code as it was before the pipeline) and as the pipeline,
        #         ALTERNATING call by call; sea_wb_denoise_ceps_utterances (there is no one-launch host call to set it against)
        # (i), (ii): device events around every step, one warm-up step of either form discarded, the steps of the forms
        # ALTERNATING in one loop, median and the sorted list of each.
        import ctypes
        lib = sea.load()
        P = lambda t: t.data_ptr() if t is not None else None
        st = torch.cuda.current_stream().cuda_stream
        steps = max(args.steps, 7)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        for wide in (False, True):
            b_all = wb_batch(batch, dev) if wide else batch
            hop = 160 if wide else 80
            n = b_all.n_utt
            lens = np.asarray(b_all.host_lengths)
            nfr = lens // hop
            frames = int(nfr.sum())
            host = b_all.data.cpu().numpy()
            utts = [host[o:o + l] for o, l in zip(b_all.host_offsets, lens)]

            class Chain:  # everything one launch group over a PackedBatch reads and writes; cap: rows of ceps per utterance
                def __init__(self, b, cap):
                    self.b = b
                    if wide:
                        half, rows = (b.total // 2 + 7) // 8 * 8, int(lib.sea_wb_rows(b.total))
                        self.out, self.f32 = z(half, torch.int16), z(half, torch.float32)
                        self.hpr, self.code = z((rows, 3), torch.float32), z((rows, 9), torch.float32)
                        self.scratch = z(int(lib.sea_wb_scratch_bytes(b.total, b.n_utt)) // 4 + 4, torch.float32)
                    else:
                        self.out, self.f32 = torch.zeros_like(b.data), z(b.data.numel(), torch.float32)
                    cum = np.concatenate(([0], np.cumsum(cap))).astype(np.int64)
                    self.tc = int(cum[-1])
                    self.ceps, self.ncep = z((max(self.tc, 1), 14), torch.float32), z(b.n_utt, torch.int32)
                    self.cum = torch.from_numpy(cum).to(dev)
            whole = Chain(b_all, np.maximum(nfr - 6, 0))
            first = torch.full((n,), -1, dtype=torch.int32, device=dev)
            onset = torch.zeros(n, dtype=torch.int32, device=dev)

            def one_launch(denoise=True, ceps=True):
                C, b = whole, b_all
                if denoise and wide:
                    rc = lib.sea_wb_denoise_batch(P(b.data), P(C.out), P(C.f32), P(b.offsets), P(b.lengths), P(b.order), P(first), P(onset),
                                                  P(C.hpr), P(C.code), P(C.scratch), b.total, n, st)
                    assert rc == 0, lib.sea_last_error()
                elif denoise:
                    rc = lib.sea_ns_denoise_batch(P(b.data), P(C.out), P(C.f32), P(b.offsets), P(b.lengths), P(b.order), P(first), n, st)
                    assert rc == 0, lib.sea_last_error()
                if ceps and wide:
                    rc = lib.sea_wb_compceps_batch(P(C.f32), P(b.offsets), P(b.lengths), P(first), P(C.hpr), P(C.code), P(C.cum), C.tc,
                                                   P(C.ceps), P(C.ncep), n, st)
                    assert rc == 0, lib.sea_last_error()
                elif ceps:
                    rc = lib.sea_compceps_batch(P(C.f32), P(b.offsets), P(b.lengths), P(first), P(C.cum), C.tc, P(C.ceps), P(C.ncep), n, st)
                    assert rc == 0, lib.sea_last_error()
            idx = np.argsort(-nfr, kind="stable")
            snfr = nfr[idx]
            state = z((n, int(lib.sea_wb_slice_state_floats() if wide else lib.sea_ns_slice_state_floats())), torch.float32)
            ccst = z((n, int(lib.sea_wb_cc_slice_state_floats() if wide else lib.sea_cc_slice_state_floats())), torch.float32)
            sfirst, sonset = torch.full_like(first, -1), torch.zeros_like(onset)
            bounds = [0]
            for k in range(1, 8):  # boundaries with equal shares of the frames, as the host pipeline cuts
                share = frames * k // 8
                f = next(f for f in range(bounds[-1] + 1, int(snfr[0]) + 1) if int(np.minimum(snfr, f).sum()) >= share)
                if f >= snfr[0]:
                    break
                bounds.append(f)
            bounds.append(int(snfr[0]))
            pieces = []
            for b0, b1 in zip(bounds[:-1], bounds[1:]):
                act = [int(u) for u in idx[snfr > b0]]
                fr = np.array([min(b1, int(nfr[u])) - b0 for u in act], np.int64)
                pb = sea.PackedBatch.from_arrays([utts[u][hop * b0:hop * min(b1, int(nfr[u]))] for u in act], dev)
                pieces.append((b0, Chain(pb, fr)))

            def run_slices(denoise=True, ceps=True):
                for k, (b0, C) in enumerate(pieces):
                    b = C.b
                    if denoise and wide:
                        rc = lib.sea_wb_denoise_batch_slice(P(b.data), P(C.out), P(C.f32), P(b.offsets), P(b.lengths), P(b.order), P(sfirst),
                                                            P(sonset), P(C.hpr), P(C.code), P(C.scratch), b.total, P(state), b.n_utt, b0,
                                                            1 if k else 0, st)
                        assert rc == 0, lib.sea_last_error()
                    elif denoise:
                        rc = lib.sea_ns_denoise_batch_slice(P(b.data), P(C.out), P(C.f32), P(b.offsets), P(b.lengths), P(b.order), P(sfirst),
                                                            P(state), b.n_utt, b0, 1 if k else 0, st)
                        assert rc == 0, lib.sea_last_error()
                    if ceps and wide:
                        rc = lib.sea_wb_compceps_batch_slice(P(C.f32), P(b.offsets), P(b.lengths), P(sfirst), P(C.hpr), P(C.code), P(C.cum),
                                                             C.tc, P(C.ceps), P(C.ncep), P(ccst), b.n_utt, b0, 1 if k else 0, st)
                        assert rc == 0, lib.sea_last_error()
                    elif ceps:
                        rc = lib.sea_compceps_batch_slice(P(C.f32), P(b.offsets), P(b.lengths), P(sfirst), P(C.cum), C.tc, P(C.ceps),
                                                          P(C.ncep), P(ccst), b.n_utt, b0, 1 if k else 0, st)
                        assert rc == 0, lib.sea_last_error()
            k8 = f"{len(pieces)} slices"
            forms = [("one launch group", one_launch), (k8, run_slices),
                     ("one launch group, denoise alone", lambda: one_launch(ceps=False)),
                     ("one launch group, compceps alone", lambda: one_launch(denoise=False)),
                     ("slices, denoise alone", lambda: run_slices(ceps=False)),
                     ("slices, compceps alone", lambda: run_slices(denoise=False))]
            for _, fn in forms:
                fn()
            torch.cuda.synchronize()
            ev = {name: [] for name, _ in forms}
            for _ in range(steps):
                for name, fn in forms:
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fn()
                    b.record()
                    ev[name].append((a, b))
            torch.cuda.synchronize()
            run_slices()  # the whole chain once more after the steps alone, for the comparison of the counts below
            torch.cuda.synchronize()
            rows = int(whole.ncep.sum().item())
            assert sum(int(C.ncep.sum().item()) for _, C in pieces) == rows, "the slices' cepstral frames do not sum to the one launch's"
            med, srt = {}, {}
            for name, _ in forms:
                t = sorted(a.elapsed_time(b) for a, b in ev[name])
                med[name], srt[name] = t[len(t) // 2], [round(v, 3) for v in t]
            outs = [np.zeros(int(f) * 80 if wide else int(l), np.int16) for f, l in zip(nfr, lens)]
            cepss = [np.zeros((max(int(f) - 6, 1), 14), np.float32) for f in nfr]
            ptr = lambda arrs: (ctypes.c_void_p * n)(*[x.ctypes.data for x in arrs])
            pin, pout, pceps = ptr(utts), ptr(outs), ptr(cepss)
            plen = (ctypes.c_long * n)(*[int(l) for l in lens])
            pnc = (ctypes.c_int * n)()
            call = lib.sea_wb_denoise_ceps_utterances if wide else lib.sea_denoise_ceps_utterances
            modes = [("pipeline", None)] if wide else [("one launch each", "0"), ("pipeline", None)]
            saved = os.environ.pop("SEA_HOST_CEPS_PIPELINE", None)
            hostt, hostk = {m: [] for m, _ in modes}, {}
            for rep in range(steps + 1):  # the first call of either mode is the warm-up
                for m, env in modes:
                    if env is not None:
                        os.environ["SEA_HOST_CEPS_PIPELINE"] = env
                    t0 = time.perf_counter()
                    rc = call(pin, pout, pceps, pnc, plen, n)
                    dt = (time.perf_counter() - t0) * 1e3
                    os.environ.pop("SEA_HOST_CEPS_PIPELINE", None)
                    assert rc == 0, lib.sea_last_error()
                    assert sum(pnc) == rows, f"the host call's cepstral frames ({m}) are not the one launch's"
                    hostk[m] = int(lib.sea_host_last_slices())
                    if rep:
                        hostt[m].append(dt)
            if saved is not None:
                os.environ["SEA_HOST_CEPS_PIPELINE"] = saved
            hostres = {m: (sorted(t)[len(t) // 2], [round(v, 3) for v in sorted(t)]) for m, t in hostt.items()}
            one = med["one launch group"]
            cfg = {"slices": len(pieces), "one_launch_group_ms": one, "one_launch_group_ms_sorted": srt["one launch group"],
                   "slices_ms": med[k8], "slices_ms_sorted": srt[k8], "ratio_to_one_launch_group": round(med[k8] / one, 3),
                   "denoise_alone_ms": {"one_launch_group": med["one launch group, denoise alone"], "slices": med["slices, denoise alone"],
                                        "one_launch_group_sorted": srt["one launch group, denoise alone"],
                                        "slices_sorted": srt["slices, denoise alone"]},
                   "compceps_alone_ms": {"one_launch_group": med["one launch group, compceps alone"], "slices": med["slices, compceps alone"],
                                         "one_launch_group_sorted": srt["one launch group, compceps alone"],
                                         "slices_sorted": srt["slices, compceps alone"]},
                   "host_pipeline_ms": hostres["pipeline"][0], "host_pipeline_ms_sorted": hostres["pipeline"][1],
                   "host_pipeline_slices": hostk["pipeline"], "host_threads": lib.sea_host_threads()}
            if not wide:
                cfg.update({"host_one_launch_each_ms": hostres["one launch each"][0],
                            "host_one_launch_each_ms_sorted": hostres["one launch each"][1],
                            "host_one_launch_each_slices": hostk["one launch each"]})
            cfg["workload"] = (f"{n} utterances at 16 kHz: the {args.utts}-utterance corpus + as many wideband signals of the same lengths"
                               if wide else f"the {args.utts}-utterance corpus at 8 kHz") + \
                f", {frames} frames, {rows} cepstral frames; device forms: median of {steps} alternating steps after one warm-up; " \
                f"host calls: wall clock, median of {steps} alternating calls after one warm-up each"
            print(json.dumps({
                "metric": ("ETSI wideband" if wide else "8 kHz") + " NoiseSup + plain CompCeps in time slices: one launch group | slices | "
                          f"host pipeline (frames of {hop} samples/sec)",
                "value": frames / (med[k8] / 1e3), "unit": "frames/s", "ms_per_step": med[k8], "config": cfg,
                "kernels": ("per slice: sea::wb_qmf_slice_kernel + sea::ns_denoise_pipe_wb_slice_kernel + sea::wb_hb_slice_kernel + "
                            "sea::wb_slice_end_kernel + sea::compceps_wb_slice_kernel + sea::compceps_carry_slice_kernel" if wide else
                            "per slice: sea::ns_denoise_pipe_slice_kernel or sea::ns_denoise_pipe_big_slice_kernel + "
                            "sea::compceps_slice_kernel + sea::compceps_carry_slice_kernel")}), flush=True)
            del whole, pieces

    if "trainset" in what:
        # The training-set builder on the --utts corpus, noise stretches from four synthetic recordings, side by side in one
        # process (median of --steps alternating steps after one warm-up, device events): (a) the mix alone, (b) subband_batch x2
        # + irm_target_batch as three calls -- taken twice per round, b and b_again, whose difference is the run-to-run spread --,
        # (c) sea_trainset_batch without and with the noisy subbands, (d) make_trainset from host buffers (wall clock, PCIe
        # inclusive, noisy + IRM only).  The yardstick for (c) is (a) + (b).
        import ctypes
        from speech_enhancement_amd import _lib
        lib = sea.load()
        n = batch.n_utt
        lens = np.asarray(batch.host_lengths)
        recs = [(corpus.synth_utterance(900 + k, 16000 * 8).astype(np.int32) // 3).astype(np.int16) for k in range(4)]
        rec = (np.arange(n) % 4).astype(np.int32)
        off = ((np.arange(n) * 7919) % (16000 * 8 - lens + 1)).astype(np.int64)
        db = np.where(np.arange(n) % 2 == 0, 0, -5).astype(np.int32)
        base = np.arange(4, dtype=np.int64) * (16000 * 8)
        src = torch.from_numpy(np.concatenate(recs)).to(dev)
        d_start = torch.from_numpy(base[rec] + off).to(dev)
        d_snr = torch.from_numpy(sea.snr_lin(db)).to(dev)
        scaled, noisy = torch.zeros_like(batch.data), torch.zeros_like(batch.data)
        sums = torch.zeros((n, 2), dtype=torch.float32, device=dev)
        gain = torch.zeros(n, dtype=torch.float32, device=dev)
        subs = [torch.zeros(batch.total * 64, dtype=torch.int16, device=dev) for _ in range(3)]
        rows = (lens - 320) // 160 + 1
        d_rows = torch.from_numpy(np.concatenate(([0], np.cumsum(rows)[:-1])).astype(np.int64)).to(dev)
        irm = torch.zeros((int(rows.sum()), 64), dtype=torch.float32, device=dev)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        sp = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        nb = sea.PackedBatch(scaled, batch.offsets, batch.lengths, batch.order, batch.host_offsets, batch.host_lengths)

        def mix():
            _lib.check(lib.sea_addnoise_batch(p(batch.data), p(batch.offsets), p(batch.lengths), p(src), p(d_start), p(d_snr),
                                              p(scaled), p(noisy), p(sums), p(gain), n, sp()), "sea_addnoise_batch")

        def parts():
            sea.subband_batch(batch, out=subs[0])
            sea.subband_batch(nb, out=subs[1])
            _lib.check(lib.sea_irm_target_batch(p(subs[0]), p(subs[1]), p(batch.offsets), p(batch.lengths), p(d_rows), p(irm), 1,
                                                n, sp()), "sea_irm_target_batch")

        def pipeline(with_noisy):
            _lib.check(lib.sea_trainset_batch(p(batch.data), p(batch.offsets), p(batch.lengths), p(src), p(d_start), p(d_snr),
                                              p(scaled), p(noisy), p(sums), p(gain), p(subs[0]), p(subs[1]),
                                              p(subs[2]) if with_noisy else None, p(d_rows), p(irm), 1, p(batch.order), n, sp()),
                       "sea_trainset_batch")
        forms = {"a_mix": mix, "b_parts": parts, "b_parts_again": parts, "c_pipeline": lambda: pipeline(False),
                 "c_pipeline_noisy_subbands": lambda: pipeline(True)}
        for fn in forms.values():
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in forms}
        for _ in range(args.steps):
            for k, fn in forms.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                times[k].append(a.elapsed_time(b))
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        host = batch.data.cpu().numpy()
        clean = [host[o:o + l] for o, l in zip(batch.host_offsets, lens)]
        del subs, irm, scaled, noisy
        torch.cuda.empty_cache()
        sea.make_trainset(clean, recs, rec, off, db)
        hs = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            r = sea.make_trainset(clean, recs, rec, off, db)
            hs.append((time.perf_counter() - t0) * 1e3)
        samples = int(lens.sum())
        print(json.dumps({
            "metric": "training-set builder: mix | subband x2 + IRM as separate calls | sea_trainset_batch | make_trainset from host "
                      "buffers (samples/sec of the pipeline without the noisy subbands)",
            "value": samples / (med["c_pipeline"] / 1e3), "unit": "samples/s", "ms_per_step": med["c_pipeline"],
            "config": {"workload": f"the {args.utts}-utterance corpus, {samples} samples, stretches of four 8-s synthetic noise "
                                   f"recordings at 0 / -5 dB; device forms: device events, median of {args.steps} alternating steps "
                                   "after one warm-up; host call: wall clock, noisy + IRM returned",
                       "median_ms": med, "sorted_ms": {k: sorted(v) for k, v in times.items()},
                       "a_plus_b_ms": med["a_mix"] + med["b_parts"], "spread_b_ms": abs(med["b_parts"] - med["b_parts_again"]),
                       "mix_share_of_pipeline": med["a_mix"] / med["c_pipeline"],
                       "host_make_trainset_ms": sorted(hs)[len(hs) // 2], "host_make_trainset_ms_sorted": sorted(hs),
                       "host_chunks": r["chunks"]},
            "kernels": "mix_sums_kernel + mix_scale_kernel + sea::subband_kernel x2 (x3) + sea::irm_target_kernel"}), flush=True)

    if "hw25" in what:
        # The Hu-Wang estimator's front half on the 25-channel 8 kHz bank, on the --utts corpus batch taken as float samples:
        # the periphery (gammatone + hair cell + low-pass), the correlogram without and with the two ACF outputs, and the launch
        # group (periphery + correlogram without ACFs).  Device events around every step, one warm-up discarded, median.  The
        # correlogram's arithmetic is 2 x 101 x 5282 multiply-adds per frame (the window sizes sum to 5282).
        lib = sea.load()
        n = batch.n_utt
        x = batch.data.to(torch.float32)
        rows = np.asarray(batch.host_lengths, dtype=np.int64) // 80
        offs = np.concatenate(([0], np.cumsum(rows)[:-1])).astype(np.int64)
        frames = int(rows.sum())
        d_offs = torch.from_numpy(offs).to(dev)
        z = lambda shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=dev)
        hout, hev = z(batch.total * 25), z(batch.total * 25)
        cross_hc, cross_ev, pratio, mark, pitch = z((frames, 25)), z((frames, 25)), z((frames, 25)), z((frames, 25)), z(frames, torch.int32)
        acf_hc, acf_ev = z((frames, 25, 101)), z((frames, 25, 101))
        P = lambda t: t.data_ptr() if t is not None else None
        st = torch.cuda.current_stream().cuda_stream

        def periphery():
            assert lib.sea_hw25_periphery_batch(P(x), P(hout), P(hev), P(batch.offsets), P(batch.lengths), P(batch.order), n, st) == 0, lib.sea_last_error()

        def correlogram(a0=None, a1=None):
            assert lib.sea_hw25_correlogram_batch(P(hout), P(hev), P(batch.offsets), P(batch.lengths), P(d_offs), P(a0), P(a1), P(cross_hc),
                                                  P(cross_ev), P(pitch), P(pratio), P(mark), None, P(batch.order), n, st) == 0, lib.sea_last_error()

        def group():
            assert lib.sea_hw25_frontend_batch(P(x), P(hout), P(hev), P(batch.offsets), P(batch.lengths), P(d_offs), None, None, P(cross_hc),
                                               P(cross_ev), P(pitch), P(pratio), P(mark), None, P(batch.order), n, st) == 0, lib.sea_last_error()
        macs = frames * 2 * 101 * 5282
        samples = int(np.sum(batch.host_lengths))
        workload = f"the {args.utts}-utterance corpus as 8 kHz float samples: {samples} samples, {frames} frames of 80; median of {args.steps} steps after one warm-up"
        for name, fn, kernels in (("periphery (25-channel gammatone + hair cell + 91-tap low-pass)", periphery, "sea::hw25_periphery_kernel + sea::hw25_lowpass_kernel"),
                                  ("correlogram without ACF outputs", correlogram, "sea::hw25_correlogram_kernel"),
                                  ("correlogram with both ACF outputs", lambda: correlogram(acf_hc, acf_ev), "sea::hw25_correlogram_kernel"),
                                  ("launch group: periphery + correlogram without ACF outputs", group,
                                   "sea::hw25_periphery_kernel + sea::hw25_lowpass_kernel + sea::hw25_correlogram_kernel")):
            med, t = median_ms(fn, args.steps)
            line = {"metric": f"Hu-Wang front half, 25-channel 8 kHz bank: {name} (frames of 80 samples/sec); a first form, not tuned",
                    "value": frames / (med / 1e3), "unit": "frames/s", "ms_per_step": med,
                    "config": {"workload": workload, "ms_sorted": [round(v, 3) for v in t]}, "kernels": kernels}
            if "correlogram" in name:
                line["multiply_adds_per_step"] = macs
                line["multiply_adds_per_sec"] = macs / (med / 1e3)
            else:
                line["samples_per_sec"] = samples / (med / 1e3)
            print(json.dumps(line), flush=True)
        del hout, hev, acf_hc, acf_ev

    if "hw64" in what:
        # The Hu-Wang estimator's front half at 16 kHz on the 64-channel bank, on the --utts corpus batch taken as 16 kHz float
        # samples: the steps and the scheme of --what hw25.  The correlogram's arithmetic is 2 x 201 x 23396 multiply-adds per
        # frame (the window sizes sum to 23396), 8.8 times the 25-channel bank's.
        lib = sea.load()
        n = batch.n_utt
        x = batch.data.to(torch.float32)
        rows = np.asarray(batch.host_lengths, dtype=np.int64) // 160
        offs = np.concatenate(([0], np.cumsum(rows)[:-1])).astype(np.int64)
        frames = int(rows.sum())
        d_offs = torch.from_numpy(offs).to(dev)
        z = lambda shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=dev)
        hout, hev = z(batch.total * 64), z(batch.total * 64)
        cross_hc, cross_ev, pratio, mark, pitch = z((frames, 64)), z((frames, 64)), z((frames, 64)), z((frames, 64)), z(frames, torch.int32)
        acf_hc, acf_ev = z((frames, 64, 201)), z((frames, 64, 201))
        P = lambda t: t.data_ptr() if t is not None else None
        st = torch.cuda.current_stream().cuda_stream

        def periphery():
            assert lib.sea_hw64_periphery_batch(P(x), P(hout), P(hev), None, P(batch.offsets), P(batch.lengths), P(batch.order), n, st) == 0, lib.sea_last_error()

        def correlogram(a0=None, a1=None):
            assert lib.sea_hw64_correlogram_batch(P(hout), P(hev), P(batch.offsets), P(batch.lengths), P(d_offs), P(a0), P(a1), P(cross_hc),
                                                  P(cross_ev), P(pitch), P(pratio), P(mark), None, P(batch.order), n, st) == 0, lib.sea_last_error()

        def group():
            assert lib.sea_hw64_frontend_batch(P(x), P(hout), P(hev), P(batch.offsets), P(batch.lengths), P(d_offs), None, None, P(cross_hc),
                                               P(cross_ev), P(pitch), P(pratio), P(mark), None, P(batch.order), n, st) == 0, lib.sea_last_error()
        macs = frames * 2 * 201 * 23396
        samples = int(np.sum(batch.host_lengths))
        workload = (f"the {args.utts}-utterance corpus as 16 kHz float samples: {samples} samples, {frames} frames of 160, "
                    f"{lib.sea_hw64_workgroups_per_utterance(n)} workgroup(s) per utterance; median of {args.steps} steps after one warm-up")
        for name, fn, kernels in (("periphery (64-channel gammatone + hair cell + 181-tap low-pass)", periphery, "sea::hw64_periphery_kernel + sea::hw64_lowpass_kernel"),
                                  ("correlogram without ACF outputs", correlogram, "sea::hw64_correlogram_kernel"),
                                  ("correlogram with both ACF outputs", lambda: correlogram(acf_hc, acf_ev), "sea::hw64_correlogram_kernel"),
                                  ("launch group: periphery + correlogram without ACF outputs", group,
                                   "sea::hw64_periphery_kernel + sea::hw64_lowpass_kernel + sea::hw64_correlogram_kernel")):
            med, t = median_ms(fn, args.steps)
            line = {"metric": f"Hu-Wang front half, 64-channel 16 kHz bank: {name} (frames of 160 samples/sec); a first form, not tuned",
                    "value": frames / (med / 1e3), "unit": "frames/s", "ms_per_step": med,
                    "config": {"workload": workload, "ms_sorted": [round(v, 3) for v in t]}, "kernels": kernels}
            if "correlogram" in name:
                line["multiply_adds_per_step"] = macs
                line["multiply_adds_per_sec"] = macs / (med / 1e3)
            else:
                line["samples_per_sec"] = samples / (med / 1e3)
            print(json.dumps(line), flush=True)
        del hout, hev, acf_hc, acf_ev

    if "hw25pitch" in what:
        # The Hu-Wang estimator's initial grouping and pitch tracking (initGroup, pitchDtm) on the --utts corpus batch taken as
        # float samples, beside the front half that feeds it, in one process: the front half with the corrHc ACF output, the
        # correlogram alone with that output, and sea_hw25_pitch_batch without and with the stage block.  Device events around
        # every step, one warm-up discarded, median.
        lib = sea.load()
        n = batch.n_utt
        x = batch.data.to(torch.float32)
        rows = np.asarray(batch.host_lengths, dtype=np.int64) // 80
        offs = np.concatenate(([0], np.cumsum(rows)[:-1])).astype(np.int64)
        frames = int(rows.sum())
        d_offs = torch.from_numpy(offs).to(dev)
        z = lambda shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=dev)
        hout, hev = z(batch.total * 25), z(batch.total * 25)
        cross_hc, cross_ev, pratio_in, mark, gpitch = z((frames, 25)), z((frames, 25)), z((frames, 25)), z((frames, 25)), z(frames, torch.int32)
        acf_hc = z((frames, 25, 101))
        pitch, grp, pratio, status = z(frames, torch.int32), z((frames, 25)), z((frames, 25)), z(n, torch.int32)
        stages = z(frames * 55, torch.int32)
        scratch = torch.empty(int(lib.sea_hw25_pitch_scratch_bytes(frames, n)), dtype=torch.uint8, device=dev)
        P = lambda t: t.data_ptr() if t is not None else None
        st = torch.cuda.current_stream().cuda_stream

        def front():
            assert lib.sea_hw25_frontend_batch(P(x), P(hout), P(hev), P(batch.offsets), P(batch.lengths), P(d_offs), P(acf_hc), None, P(cross_hc),
                                               P(cross_ev), P(gpitch), P(pratio_in), P(mark), None, P(batch.order), n, st) == 0, lib.sea_last_error()

        def correlogram():
            assert lib.sea_hw25_correlogram_batch(P(hout), P(hev), P(batch.offsets), P(batch.lengths), P(d_offs), P(acf_hc), None, P(cross_hc),
                                                  P(cross_ev), P(gpitch), P(pratio_in), P(mark), None, P(batch.order), n, st) == 0, lib.sea_last_error()

        def stage(with_stages=False):
            assert lib.sea_hw25_pitch_batch(P(acf_hc), P(cross_hc), P(pratio_in), P(mark), P(batch.lengths), P(d_offs), P(pitch), P(grp), P(pratio),
                                            P(status), P(stages) if with_stages else None, P(scratch), P(batch.order), n, st) == 0, lib.sea_last_error()
        samples = int(np.sum(batch.host_lengths))
        workload = f"the {args.utts}-utterance corpus as 8 kHz float samples: {samples} samples, {frames} frames of 80; median of {args.steps} steps after one warm-up"
        results = []
        for name, fn, kernels in (("front half with the corrHc ACF output", front, "sea::hw25_periphery_kernel + sea::hw25_lowpass_kernel + sea::hw25_correlogram_kernel"),
                                  ("correlogram with the corrHc ACF output", correlogram, "sea::hw25_correlogram_kernel"),
                                  ("initial grouping and pitch tracking", stage,
                                   "sea::hw25_pitch_max_kernel + _segment_kernel + _frame_kernel x3 + _regroup_kernel x2 + _track_kernel"),
                                  ("initial grouping and pitch tracking with the stage block", lambda: stage(True), "the same")):
            med, t = median_ms(fn, args.steps)
            results.append(med)
            print(json.dumps({"metric": f"Hu-Wang estimator, 25-channel 8 kHz bank: {name} (frames of 80 samples/sec); a first form, not tuned",
                              "value": frames / (med / 1e3), "unit": "frames/s", "ms_per_step": med,
                              "config": {"workload": workload, "ms_sorted": [round(v, 3) for v in t]}, "kernels": kernels}), flush=True)
        s_host = status.cpu().numpy()
        p_host = pitch.cpu().numpy()
        print(json.dumps({"metric": "Hu-Wang estimator: initial grouping and pitch tracking relative to the correlogram of the same run",
                          "value": results[2] / results[1], "unit": "ratio", "config": {"workload": workload},
                          "segments_per_utterance": {"min": int((s_host & 0xFFFF).min()), "median": float(np.median(s_host & 0xFFFF)),
                                                     "max": int((s_host & 0xFFFF).max())},
                          "utterances_flagged": {"too_many_segments": int((s_host >> 16 & 1).sum()), "chanmark_unset": int((s_host >> 17 & 1).sum())},
                          "voiced_frames": int((p_host > 0).sum())}), flush=True)
        del hout, hev, acf_hc, stages, scratch

    if "hw64pitch" in what:
        # The same stage at 16 kHz on the 64-channel bank (sea_hw64_pitch_batch) on the --utts corpus batch taken as 16 kHz float
        # samples, beside the front half that feeds it, in one process and with the scheme of --what hw25pitch.  The corpus runs
        # WHOLE: its corrHc ACF is 51 456 B per row (about 21 GB at 1024 utterances) and hOut / hEv are 256 B per sample each; the
        # total is checked against the free device memory first, and the run stops there if it does not fit.
        lib = sea.load()
        n = batch.n_utt
        rows = np.asarray(batch.host_lengths, dtype=np.int64) // 160
        offs = np.concatenate(([0], np.cumsum(rows)[:-1])).astype(np.int64)
        frames = int(rows.sum())
        scratch_bytes = int(lib.sea_hw64_pitch_scratch_bytes(frames, n))
        need = 4 * (frames * (64 * 201 + 6 * 64 + 2 + 133) + 2 * int(batch.total) * 64 + int(batch.total)) + scratch_bytes
        free, total = torch.cuda.mem_get_info()
        assert need < 0.9 * free, f"hw64pitch: the corpus whole needs {need / 1e9:.1f} GB, {free / 1e9:.1f} GB of device memory are free"
        x = batch.data.to(torch.float32)
        d_offs = torch.from_numpy(offs).to(dev)
        z = lambda shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=dev)
        hout, hev = z(batch.total * 64), z(batch.total * 64)
        cross_hc, cross_ev, pratio_in, mark, gpitch = z((frames, 64)), z((frames, 64)), z((frames, 64)), z((frames, 64)), z(frames, torch.int32)
        acf_hc = z((frames, 64, 201))
        pitch, grp, pratio, status = z(frames, torch.int32), z((frames, 64)), z((frames, 64)), z(n, torch.int32)
        stages = z(frames * 133, torch.int32)
        scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=dev)
        P = lambda t: t.data_ptr() if t is not None else None
        st = torch.cuda.current_stream().cuda_stream

        def front():
            assert lib.sea_hw64_frontend_batch(P(x), P(hout), P(hev), P(batch.offsets), P(batch.lengths), P(d_offs), P(acf_hc), None, P(cross_hc),
                                               P(cross_ev), P(gpitch), P(pratio_in), P(mark), None, P(batch.order), n, st) == 0, lib.sea_last_error()

        def correlogram():
            assert lib.sea_hw64_correlogram_batch(P(hout), P(hev), P(batch.offsets), P(batch.lengths), P(d_offs), P(acf_hc), None, P(cross_hc),
                                                  P(cross_ev), P(gpitch), P(pratio_in), P(mark), None, P(batch.order), n, st) == 0, lib.sea_last_error()

        def stage(with_stages=False):
            assert lib.sea_hw64_pitch_batch(P(acf_hc), P(pratio_in), P(mark), P(batch.lengths), P(d_offs), P(pitch), P(grp), P(pratio),
                                            P(status), P(stages) if with_stages else None, P(scratch), P(batch.order), n, st) == 0, lib.sea_last_error()
        samples = int(np.sum(batch.host_lengths))
        workload = (f"the {args.utts}-utterance corpus WHOLE as 16 kHz float samples: {samples} samples, {frames} frames of 160, "
                    f"{frames * 64 * 201 * 4 / 1e9:.1f} GB of corrHc ACF, {need / 1e9:.1f} GB of device memory in all ({free / 1e9:.0f} GB were free), "
                    f"{lib.sea_hw64_pitch_waves_per_utterance(n)} wave(s) per utterance in the frame kernels; median of {args.steps} steps after one warm-up")
        results = []
        for name, fn, kernels in (("front half with the corrHc ACF output", front, "sea::hw64_periphery_kernel + sea::hw64_lowpass_kernel + sea::hw64_correlogram_kernel"),
                                  ("correlogram with the corrHc ACF output", correlogram, "sea::hw64_correlogram_kernel"),
                                  ("initial grouping and pitch tracking", stage,
                                   "sea::hw64_pitch_max_kernel + _segment_kernel + _frame_kernel x3 + _regroup_kernel x2 + _track_kernel"),
                                  ("initial grouping and pitch tracking with the stage block", lambda: stage(True), "the same")):
            med, t = median_ms(fn, args.steps)
            results.append(med)
            print(json.dumps({"metric": f"Hu-Wang estimator, 64-channel 16 kHz bank: {name} (frames of 160 samples/sec); a first form, not tuned",
                              "value": frames / (med / 1e3), "unit": "frames/s", "ms_per_step": med,
                              "config": {"workload": workload, "ms_sorted": [round(v, 3) for v in t]}, "kernels": kernels}), flush=True)
        s_host = status.cpu().numpy()
        p_host = pitch.cpu().numpy()
        print(json.dumps({"metric": "Hu-Wang estimator, 64-channel 16 kHz bank: initial grouping and pitch tracking relative to the correlogram of the same run",
                          "value": results[2] / results[1], "unit": "ratio", "config": {"workload": workload},
                          "segments_per_utterance": {"min": int((s_host & 0xFFFF).min()), "median": float(np.median(s_host & 0xFFFF)),
                                                     "max": int((s_host & 0xFFFF).max())},
                          "utterances_flagged": {"too_many_segments": int((s_host >> 16 & 1).sum()), "chanmark_unset": int((s_host >> 17 & 1).sum())},
                          "voiced_frames": int((p_host > 0).sum()), "plus_units_in_channels_40_to_63": int((grp[:, 40:] > 0).sum().item())}), flush=True)
        del hout, hev, acf_hc, stages, scratch

    if "hw25ibm" in what:
        # The rest of the Hu-Wang estimator (computeAM, finalSeg) and the whole of createIBM on the --utts corpus batch taken as
        # float samples, beside the stages that feed them, in one process: the periphery with gOut, the correlogram with the
        # corrHc ACF output, initGroup + pitchDtm, the AM stage, the final grouping, and sea_hw25_ibm_batch.  Device events
        # around every step, one warm-up discarded, median.
        lib = sea.load()
        n = batch.n_utt
        x = batch.data.to(torch.float32)
        rows = np.asarray(batch.host_lengths, dtype=np.int64) // 80
        offs = np.concatenate(([0], np.cumsum(rows)[:-1])).astype(np.int64)
        frames, total = int(rows.sum()), int(batch.total)
        d_offs = torch.from_numpy(offs).to(dev)
        z = lambda shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=dev)
        hout, hev, gout = z(total * 25), z(total * 25), z(total * 25)
        cross_hc, cross_ev, pratio_in, mark, gpitch = z((frames, 25)), z((frames, 25)), z((frames, 25)), z((frames, 25)), z(frames, torch.int32)
        acf_hc = z((frames, 25, 101))
        pitch, grp, pratio, status = z(frames, torch.int32), z((frames, 25)), z((frames, 25)), z(n, torch.int32)
        amcrn, mask, st_am, st_fin, st_ibm, pitch2, mask2 = z((frames, 25)), z((frames, 25)), z(n, torch.int32), z(n, torch.int32), z(n, torch.int32), z(frames, torch.int32), z((frames, 25))
        scr_pitch = torch.empty(int(lib.sea_hw25_pitch_scratch_bytes(frames, n)), dtype=torch.uint8, device=dev)
        scr_am = torch.empty(int(lib.sea_hw25_am_scratch_bytes(total, n)), dtype=torch.uint8, device=dev)
        scr_fin = torch.empty(int(lib.sea_hw25_finalseg_scratch_bytes(frames, n)), dtype=torch.uint8, device=dev)
        scr_ibm = torch.empty(int(lib.sea_hw25_ibm_scratch_bytes(total, frames, n)), dtype=torch.uint8, device=dev)
        P = lambda t: t.data_ptr() if t is not None else None
        st = torch.cuda.current_stream().cuda_stream

        def periphery():
            assert lib.sea_hw25_periphery_gout_batch(P(x), P(hout), P(hev), P(gout), P(batch.offsets), P(batch.lengths), P(batch.order), n, st) == 0, lib.sea_last_error()

        def correlogram():
            assert lib.sea_hw25_correlogram_batch(P(hout), P(hev), P(batch.offsets), P(batch.lengths), P(d_offs), P(acf_hc), None, P(cross_hc),
                                                  P(cross_ev), P(gpitch), P(pratio_in), P(mark), None, P(batch.order), n, st) == 0, lib.sea_last_error()

        def pitch_stage():
            assert lib.sea_hw25_pitch_batch(P(acf_hc), P(cross_hc), P(pratio_in), P(mark), P(batch.lengths), P(d_offs), P(pitch), P(grp), P(pratio),
                                            P(status), None, P(scr_pitch), P(batch.order), n, st) == 0, lib.sea_last_error()

        def am_stage():
            assert lib.sea_hw25_am_batch(P(gout), P(pitch), P(batch.offsets), P(batch.lengths), P(d_offs), P(amcrn), None, None, None, None,
                                         P(st_am), P(scr_am), total, P(batch.order), n, st) == 0, lib.sea_last_error()

        def final_stage():
            assert lib.sea_hw25_finalseg_batch(P(grp), P(amcrn), P(cross_ev), P(pratio), P(batch.lengths), P(d_offs), P(mask), None, P(st_fin),
                                               None, P(scr_fin), P(batch.order), n, st) == 0, lib.sea_last_error()

        def whole():
            assert lib.sea_hw25_ibm_batch(P(x), P(batch.offsets), P(batch.lengths), P(d_offs), P(mask2), P(pitch2), P(st_ibm), None, P(scr_ibm),
                                          total, frames, P(batch.order), n, st) == 0, lib.sea_last_error()
        samples = int(np.sum(batch.host_lengths))
        workload = f"the {args.utts}-utterance corpus as 8 kHz float samples: {samples} samples, {frames} frames of 80; median of {args.steps} steps after one warm-up"
        results = {}
        for key, name, fn, kernels in (
                ("periphery", "periphery with gOut", periphery, "sea::hw25_periphery_kernel + sea::hw25_lowpass_kernel"),
                ("correlogram", "correlogram with the corrHc ACF output", correlogram, "sea::hw25_correlogram_kernel"),
                ("pitch", "initial grouping and pitch tracking", pitch_stage, "the eight launches of sea_hw25_pitch_batch"),
                ("am", "AM stage (amPatt, hilbert, computeAMRate)", am_stage,
                 "sea::hw25_am_prepare_kernel + _patt_kernel + per channel group (_fft_head_kernel + 6 x _fft_stage_kernel) x 2 + _norm_kernel; _rate_kernel"),
                ("final", "final grouping (finalSeg)", final_stage, "sea::hw25_finalseg_kernel"),
                ("whole", "the whole estimator, sea_hw25_ibm_batch", whole, "all of the above")):
            med, t = median_ms(fn, args.steps)
            results[key] = med
            print(json.dumps({"metric": f"Hu-Wang estimator, 25-channel 8 kHz bank: {name} (frames of 80 samples/sec); a first form, not tuned",
                              "value": frames / (med / 1e3), "unit": "frames/s", "ms_per_step": med,
                              "config": {"workload": workload, "ms_sorted": [round(v, 3) for v in t]}, "kernels": kernels}), flush=True)
        assert torch.equal(mask, mask2) and torch.equal(pitch, pitch2), "the launch group and the single stages differ"
        s_host = (st_ibm.cpu().numpy() | st_am.cpu().numpy() | st_fin.cpu().numpy())
        print(json.dumps({"metric": "Hu-Wang estimator: each stage relative to the correlogram of the same run",
                          "value": results["whole"] / results["correlogram"], "unit": "ratio (the whole estimator)",
                          "stage_over_correlogram": {k: v / results["correlogram"] for k, v in results.items()},
                          "config": {"workload": workload, "fft_channels_per_launch_group": 25 if total * 2 * 25 * 16 <= (256 << 20) else 5},
                          "utterances_flagged": {"final_too_many_segments": int((s_host >> 18 & 1).sum()), "am_too_long": int((s_host >> 19 & 1).sum())},
                          "voiced_frames": int((pitch.cpu().numpy() > 0).sum()), "am_labels": int(amcrn.sum().item()),
                          "mask_units": int(mask.sum().item())}), flush=True)
        del hout, hev, gout, acf_hc, scr_am, scr_ibm

    if "hw64ibm" in what:
        # The rest of the Hu-Wang estimator at 16 kHz on the 64-channel bank (computeAM, finalSeg) and the whole of createIBM on
        # the --utts corpus batch taken as 16 kHz float samples, beside the stages that exist, in one process and with the scheme
        # of --what hw25ibm: the periphery with the gOut store, the correlogram with the corrHc ACF output, initGroup + pitchDtm,
        # the AM stage, the final grouping, and sea_hw64_ibm_batch.  Device events around every step, one warm-up discarded,
        # median.  The single stages need three sample streams of 256 B per sample, the ACF of 51 456 B per row and the AM
        # scratch (two more streams and the FFT's buffers); the launch group keeps all of that in its own scratch, so the stages'
        # buffers are freed before it is allocated.  The larger of the two is checked against the free device memory BEFORE
        # anything is allocated; if the corpus whole does not fit, its first half, quarter, ... runs, and the lines say so.
        # The lines also go to profiles/hw64ibm_bench_extra.jsonl.
        lib = sea.load()

        def plan(k):
            lengths = np.array([corpus.utterance_length(u) for u in range(k)], dtype=np.int64)
            _, tot, _ = sea.PackedBatch.layout(lengths)
            fr = int((lengths // 160).sum())
            stage_bytes = (4 * (3 * tot * 64 + fr * 64 * 201 + 13 * fr * 64 + 3 * fr) + int(lib.sea_hw64_pitch_scratch_bytes(fr, k))
                           + int(lib.sea_hw64_am_scratch_bytes(tot, k)) + int(lib.sea_hw64_finalseg_scratch_bytes(fr, k)))
            group_bytes = int(lib.sea_hw64_ibm_scratch_bytes(tot, fr, k)) + 4 * (2 * fr * 64 + 2 * fr)
            return max(stage_bytes, group_bytes) + 4 * int(tot)

        free, _ = torch.cuda.mem_get_info()
        n = args.utts
        while n > 1 and plan(n) >= 0.9 * free:
            n //= 2
        need = plan(n)
        assert need < 0.9 * free, f"hw64ibm: one utterance needs {need / 1e9:.1f} GB, {free / 1e9:.1f} GB of device memory are free"
        shard = batch if n == args.utts else bench.build_shard(n, 0, dev)
        x = shard.data.to(torch.float32)
        rows = np.asarray(shard.host_lengths, dtype=np.int64) // 160
        offs = np.concatenate(([0], np.cumsum(rows)[:-1])).astype(np.int64)
        frames, total = int(rows.sum()), int(shard.total)
        d_offs = torch.from_numpy(offs).to(dev)
        z = lambda shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=dev)
        hout, hev, gout = z(total * 64), z(total * 64), z(total * 64)
        cross_hc, cross_ev, pratio_in, mark, gpitch = z((frames, 64)), z((frames, 64)), z((frames, 64)), z((frames, 64)), z(frames, torch.int32)
        acf_hc = z((frames, 64, 201))
        pitch, grp, pratio, status = z(frames, torch.int32), z((frames, 64)), z((frames, 64)), z(n, torch.int32)
        amcrn, mask, st_am, st_fin, st_ibm, pitch2, mask2 = z((frames, 64)), z((frames, 64)), z(n, torch.int32), z(n, torch.int32), z(n, torch.int32), z(frames, torch.int32), z((frames, 64))
        scr_pitch = torch.empty(int(lib.sea_hw64_pitch_scratch_bytes(frames, n)), dtype=torch.uint8, device=dev)
        scr_am = torch.empty(int(lib.sea_hw64_am_scratch_bytes(total, n)), dtype=torch.uint8, device=dev)
        scr_fin = torch.empty(int(lib.sea_hw64_finalseg_scratch_bytes(frames, n)), dtype=torch.uint8, device=dev)
        P = lambda t: t.data_ptr() if t is not None else None
        st = torch.cuda.current_stream().cuda_stream
        order = shard.order

        def periphery(with_gout=True):
            assert lib.sea_hw64_periphery_batch(P(x), P(hout), P(hev), P(gout) if with_gout else None, P(shard.offsets), P(shard.lengths), P(order), n, st) == 0, lib.sea_last_error()

        def correlogram():
            assert lib.sea_hw64_correlogram_batch(P(hout), P(hev), P(shard.offsets), P(shard.lengths), P(d_offs), P(acf_hc), None, P(cross_hc),
                                                  P(cross_ev), P(gpitch), P(pratio_in), P(mark), None, P(order), n, st) == 0, lib.sea_last_error()

        def pitch_stage():
            assert lib.sea_hw64_pitch_batch(P(acf_hc), P(pratio_in), P(mark), P(shard.lengths), P(d_offs), P(pitch), P(grp), P(pratio),
                                            P(status), None, P(scr_pitch), P(order), n, st) == 0, lib.sea_last_error()

        def am_stage():
            assert lib.sea_hw64_am_batch(P(gout), P(pitch), P(shard.offsets), P(shard.lengths), P(d_offs), P(amcrn), None, None, None, None,
                                         P(st_am), P(scr_am), total, P(order), n, st) == 0, lib.sea_last_error()

        def final_stage():
            assert lib.sea_hw64_finalseg_batch(P(grp), P(amcrn), P(cross_ev), P(pratio), P(shard.lengths), P(d_offs), P(mask), None, P(st_fin),
                                               None, P(scr_fin), P(order), n, st) == 0, lib.sea_last_error()
        samples = int(np.sum(shard.host_lengths))
        chunk = 64 if total * 2 * 64 * 16 <= (256 << 20) else 8
        part = "WHOLE" if n == args.utts else f"FIRST {n} UTTERANCES ONLY (the whole does not fit)"
        workload = (f"the {args.utts}-utterance corpus, {part}, as 16 kHz float samples: {samples} samples, {frames} frames of 160, "
                    f"{need / 1e9:.1f} GB of device memory at the most ({free / 1e9:.0f} GB were free), the FFT over {chunk} channels per launch "
                    f"group; median of {args.steps} steps after one warm-up")
        out_path = os.path.join(ROOT, "profiles", "hw64ibm_bench_extra.jsonl")
        lines = []

        def emit(record):
            lines.append(json.dumps(record))
            print(lines[-1], flush=True)

        results = {}

        def measure(key, name, fn, kernels):
            med, t = median_ms(fn, args.steps)
            results[key] = med
            emit({"metric": f"Hu-Wang estimator, 64-channel 16 kHz bank: {name} (frames of 160 samples/sec); a first form, not tuned",
                  "value": frames / (med / 1e3), "unit": "frames/s", "ms_per_step": med,
                  "config": {"workload": workload, "ms_sorted": [round(v, 3) for v in t]}, "kernels": kernels})

        measure("periphery_plain", "periphery without gOut", lambda: periphery(False), "sea::hw64_periphery_kernel + sea::hw64_lowpass_kernel")
        measure("periphery", "periphery with the gOut store", periphery, "sea::hw64_periphery_kernel + sea::hw64_lowpass_kernel")
        measure("correlogram", "correlogram with the corrHc ACF output", correlogram, "sea::hw64_correlogram_kernel")
        measure("pitch", "initial grouping and pitch tracking", pitch_stage, "the eight launches of sea_hw64_pitch_batch")
        measure("am", "AM stage (amPatt, hilbert, computeAMRate)", am_stage,
                "sea::hw64_am_prepare_kernel + _patt_kernel + per channel group (_fft_head_kernel + 6 x _fft_stage_kernel) x 2 + _norm_kernel; _rate_kernel")
        measure("final", "final grouping (finalSeg)", final_stage, "sea::hw64_finalseg_kernel")
        del hout, hev, gout, acf_hc, scr_am, scr_pitch, scr_fin
        torch.cuda.empty_cache()
        scr_ibm = torch.empty(int(lib.sea_hw64_ibm_scratch_bytes(total, frames, n)), dtype=torch.uint8, device=dev)

        def whole():
            assert lib.sea_hw64_ibm_batch(P(x), P(shard.offsets), P(shard.lengths), P(d_offs), P(mask2), P(pitch2), P(st_ibm), None, P(scr_ibm),
                                          total, frames, P(order), n, st) == 0, lib.sea_last_error()
        measure("whole", "the whole estimator, sea_hw64_ibm_batch", whole, "all of the above")
        assert torch.equal(mask, mask2) and torch.equal(pitch, pitch2), "the launch group and the single stages differ"
        s_host = (st_ibm.cpu().numpy() | st_am.cpu().numpy() | st_fin.cpu().numpy())
        emit({"metric": "Hu-Wang estimator, 64-channel 16 kHz bank: each stage relative to the correlogram of the same run",
              "value": results["whole"] / results["correlogram"], "unit": "ratio (the whole estimator)",
              "stage_over_correlogram": {k: v / results["correlogram"] for k, v in results.items()},
              "config": {"workload": workload, "fft_channels_per_launch_group": chunk},
              "utterances_flagged": {"final_too_many_segments": int((s_host >> 18 & 1).sum()), "am_too_long": int((s_host >> 19 & 1).sum()),
                                     "am_bad_pitch": int((s_host >> 20 & 1).sum())},
              "voiced_frames": int((pitch.cpu().numpy() > 0).sum()), "am_labels": int(amcrn.sum().item()),
              "am_labels_in_channels_40_to_63": int(amcrn[:, 40:].sum().item()), "mask_units": int(mask.sum().item())})
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        del scr_ibm

    if "hw25resynth" in what:
        # The Hu-Wang resynthesis on the --utts corpus batch taken as float samples, in one process: sea_hw25_resynth_batch alone
        # (float output, on the gOut and the mask of the same run), sea_hw25_enhance_batch (audio in, enhanced audio out), and
        # beside them sea_hw25_ibm_batch and the periphery with gOut, whose kernel runs the same recurrence.  Device events around
        # every step, one warm-up discarded, median.
        lib = sea.load()
        n = batch.n_utt
        x = batch.data.to(torch.float32)
        rows = np.asarray(batch.host_lengths, dtype=np.int64) // 80
        offs = np.concatenate(([0], np.cumsum(rows)[:-1])).astype(np.int64)
        frames, total = int(rows.sum()), int(batch.total)
        d_offs = torch.from_numpy(offs).to(dev)
        z = lambda shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=dev)
        hout, hev, gout = z(total * 25), z(total * 25), z(total * 25)
        mask, pitch, status = z((frames, 25)), z(frames, torch.int32), z(n, torch.int32)
        mask2, pitch2, status2 = z((frames, 25)), z(frames, torch.int32), z(n, torch.int32)
        audio, audio2, shorts = z(total), z(total), z(total, torch.int16)
        scr_ibm = torch.empty(int(lib.sea_hw25_ibm_scratch_bytes(total, frames, n)), dtype=torch.uint8, device=dev)
        P = lambda t: t.data_ptr() if t is not None else None
        st = torch.cuda.current_stream().cuda_stream

        def periphery():
            assert lib.sea_hw25_periphery_gout_batch(P(x), P(hout), P(hev), P(gout), P(batch.offsets), P(batch.lengths), P(batch.order), n, st) == 0, lib.sea_last_error()

        def ibm():
            assert lib.sea_hw25_ibm_batch(P(x), P(batch.offsets), P(batch.lengths), P(d_offs), P(mask), P(pitch), P(status), None, P(scr_ibm),
                                          total, frames, P(batch.order), n, st) == 0, lib.sea_last_error()

        def resynth(i16=None):
            assert lib.sea_hw25_resynth_batch(P(gout), P(mask), P(batch.offsets), P(batch.lengths), P(d_offs), 0.0, P(audio), P(i16),
                                              P(batch.order), n, st) == 0, lib.sea_last_error()

        def enhance():
            assert lib.sea_hw25_enhance_batch(P(x), P(batch.offsets), P(batch.lengths), P(d_offs), P(audio2), None, P(mask2), P(pitch2),
                                              P(status2), P(scr_ibm), total, frames, P(batch.order), n, st) == 0, lib.sea_last_error()
        samples = int(np.sum(batch.host_lengths))
        workload = f"the {args.utts}-utterance corpus as 8 kHz float samples: {samples} samples, {frames} frames of 80; median of {args.steps} steps after one warm-up"
        results = {}
        for key, name, fn, kernels in (
                ("periphery", "periphery with gOut", periphery, "sea::hw25_periphery_kernel + sea::hw25_lowpass_kernel"),
                ("ibm", "the whole estimator, sea_hw25_ibm_batch", ibm, "every kernel of the estimator"),
                ("resynth", "resynthesis alone, float output", resynth, "sea::hw25_resynth_kernel"),
                ("resynth_i16", "resynthesis alone, float and int16 outputs", lambda: resynth(shorts), "sea::hw25_resynth_kernel"),
                ("enhance", "audio in, enhanced audio out, sea_hw25_enhance_batch", enhance, "every kernel of the estimator + sea::hw25_resynth_kernel")):
            med, t = median_ms(fn, args.steps)
            results[key] = med
            print(json.dumps({"metric": f"Hu-Wang 25-channel resynthesis: {name} (samples/sec); a first form, not tuned",
                              "value": samples / (med / 1e3), "unit": "samples/s", "ms_per_step": med, "x_realtime_8k": samples / 8000.0 / (med / 1e3),
                              "config": {"workload": workload, "ms_sorted": [round(v, 3) for v in t]}, "kernels": kernels}), flush=True)
        assert torch.equal(mask, mask2) and torch.equal(audio.view(torch.int32), audio2.view(torch.int32)), "the launch group and the single stages differ"
        print(json.dumps({"metric": "Hu-Wang 25-channel resynthesis relative to the periphery and to the estimator of the same run",
                          "value": results["resynth"] / results["periphery"], "unit": "ratio (resynthesis / periphery with gOut)",
                          "resynth_over_ibm": results["resynth"] / results["ibm"], "enhance_over_ibm": results["enhance"] / results["ibm"],
                          "config": {"workload": workload}, "mask_units": int(mask.sum().item()),
                          "nonzero_output_samples": int((audio != 0).sum().item())}), flush=True)
        del hout, hev, gout, scr_ibm

    if "hw64resynth" in what:
        # The Hu-Wang resynthesis at 16 kHz on the 64-channel bank, on the --utts corpus batch taken as 16 kHz float samples, in
        # one process.  Through the exported device-pointer calls, device events around every step: the periphery with gOut and
        # sea_hw64_ibm_batch.  The resynthesis has no exported device-pointer call: it is reached through the host-list forms,
        # which time their own resynthesis launches with a pair of device events (sea_hw64_enhance_last_resynth_ms): that is
        # "the resynthesis alone"; the host calls' wall time (upload, launch group, download) is given beside it.  One warm-up
        # discarded, median of --steps.  The launch group's audio and mask are checked against the single stages, bit for bit.
        # The lines also go to profiles/hw64resynth_bench_extra.jsonl.
        import ctypes
        lib = sea.load()
        n = batch.n_utt
        x = batch.data.to(torch.float32)
        lengths = np.asarray(batch.host_lengths, dtype=np.int64)
        rows = lengths // 160
        offs = np.concatenate(([0], np.cumsum(rows)[:-1])).astype(np.int64)
        frames, total, samples = int(rows.sum()), int(batch.total), int(lengths.sum())
        d_offs = torch.from_numpy(offs).to(dev)
        z = lambda shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=dev)
        hout, hev, gout = z(total * 64), z(total * 64), z(total * 64)
        mask, pitch, status = z((frames, 64)), z(frames, torch.int32), z(n, torch.int32)
        scr_ibm = torch.empty(int(lib.sea_hw64_ibm_scratch_bytes(total, frames, n)), dtype=torch.uint8, device=dev)
        P = lambda t: t.data_ptr() if t is not None else None
        st = torch.cuda.current_stream().cuda_stream

        def periphery():
            assert lib.sea_hw64_periphery_batch(P(x), P(hout), P(hev), P(gout), P(batch.offsets), P(batch.lengths), P(batch.order), n, st) == 0, lib.sea_last_error()

        def ibm():
            assert lib.sea_hw64_ibm_batch(P(x), P(batch.offsets), P(batch.lengths), P(d_offs), P(mask), P(pitch), P(status), None, P(scr_ibm),
                                          total, frames, P(batch.order), n, st) == 0, lib.sea_last_error()
        workload = (f"the {args.utts}-utterance corpus as 16 kHz float samples: {samples} samples, {frames} frames of 160; median of "
                    f"{args.steps} steps after one warm-up")
        lines, results = [], {}

        def emit(record):
            lines.append(json.dumps(record))
            print(lines[-1], flush=True)

        def line(key, name, med, t, kernels, **more):
            results[key] = med
            emit({"metric": f"Hu-Wang 64-channel 16 kHz resynthesis: {name} (samples/sec); a first form, not tuned",
                  "value": samples / (med / 1e3), "unit": "samples/s", "ms_per_step": med, "x_realtime_16k": samples / 16000.0 / (med / 1e3),
                  "config": {"workload": workload, "ms_sorted": [round(v, 3) for v in t]}, "kernels": kernels, **more})

        for key, name, fn, kernels in (("periphery", "periphery with gOut, device events", periphery, "sea::hw64_periphery_kernel + sea::hw64_lowpass_kernel"),
                                       ("ibm", "the whole estimator, sea_hw64_ibm_batch, device events", ibm, "every kernel of the estimator")):
            med, t = median_ms(fn, args.steps)
            line(key, name, med, t, kernels)
        torch.cuda.synchronize()
        host = x.cpu().numpy()
        xs = [np.ascontiguousarray(host[int(o):int(o) + int(L)]) for o, L in zip(batch.host_offsets, lengths)]
        mask_h, pitch_h = mask.cpu().numpy(), pitch.cpu().numpy()
        masks = [np.ascontiguousarray(mask_h[int(o):int(o) + int(r)]) for o, r in zip(offs, rows)]
        del hout, hev, gout, scr_ibm
        torch.cuda.empty_cache()
        ptrs = lambda arrs: (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs]) if arrs is not None else None
        lens = (ctypes.c_long * n)(*[int(L) for L in lengths])
        audio = [np.zeros(int(L), np.float32) for L in lengths]
        audio2 = [np.zeros(int(L), np.float32) for L in lengths]
        shorts = [np.zeros(int(L), np.int16) for L in lengths]
        masks2 = [np.zeros((int(r), 64), np.float32) for r in rows]
        pitch2 = [np.zeros(int(r), np.int32) for r in rows]
        status2 = np.zeros(n, np.int32)

        def host_call(fn):
            """one warm-up, then --steps calls -> (the launches' device time, the calls' wall time, chunks), medians in ms"""
            dev_ms, wall_ms = [], []
            for i in range(args.steps + 1):
                t0 = time.perf_counter()
                assert fn() == 0, lib.sea_last_error()
                if i:
                    wall_ms.append((time.perf_counter() - t0) * 1e3)
                    dev_ms.append(float(lib.sea_hw64_enhance_last_resynth_ms()))
            return sorted(dev_ms), sorted(wall_ms), int(lib.sea_hw64_enhance_last_chunks())

        def resynth_call(i16):
            return lambda: lib.sea_hw64_resynth_utterances(ptrs(xs), lens, ptrs(masks), 0.0, ptrs(audio), ptrs(shorts) if i16 else None, n)

        def enhance_call():
            return lib.sea_hw64_enhance_utterances(ptrs(xs), lens, n, ptrs(audio2), None, ptrs(masks2), ptrs(pitch2),
                                                   status2.ctypes.data_as(ctypes.c_void_p))
        for key, name, fn in (("resynth", "resynthesis alone, float output", resynth_call(False)),
                              ("resynth_i16", "resynthesis alone, float and int16 outputs", resynth_call(True))):
            d, w, chunks = host_call(fn)
            line(key, name + ": the launches inside sea_hw64_resynth_utterances, device events", d[len(d) // 2], d, "sea::hw64_resynth_kernel",
                 host_call_wall_ms=w[len(w) // 2], host_call_wall_ms_sorted=[round(v, 1) for v in w], chunks=chunks)
        d, w, chunks = host_call(enhance_call)
        line("enhance", "audio in, enhanced audio out, sea_hw64_enhance_utterances end to end from host memory, wall time", w[len(w) // 2], w,
             "every kernel of the estimator + sea::hw64_resynth_kernel, with the upload and the download", chunks=chunks,
             resynth_launch_ms=d[len(d) // 2])
        same_audio = all(a.tobytes() == b.tobytes() for a, b in zip(audio, audio2))
        same_mask = all(np.array_equal(a, b) for a, b in zip(masks, masks2)) and np.array_equal(np.concatenate(pitch2), pitch_h)
        assert same_audio and same_mask, "the launch group and the single stages differ"
        emit({"metric": "Hu-Wang 64-channel 16 kHz resynthesis relative to the periphery and to the estimator of the same run",
              "value": results["resynth"] / results["periphery"], "unit": "ratio (resynthesis / periphery with gOut)",
              "resynth_over_ibm": results["resynth"] / results["ibm"], "enhance_host_call_over_ibm": results["enhance"] / results["ibm"],
              "config": {"workload": workload}, "chunks": chunks, "audio_and_mask_equal_the_single_stages": True,
              "mask_units": int(mask_h.sum()), "nonzero_output_samples": int(sum(int((a != 0).sum()) for a in audio))})
        with open(os.path.join(ROOT, "profiles", "hw64resynth_bench_extra.jsonl"), "w") as fh:
            fh.write("\n".join(lines) + "\n")

    if "dnn" in what:
        # The DNN mask estimator on the --utts corpus batch taken as 16 kHz int16 utterances, with a seeded 704-1024-1024-1024-64
        # sigmoid network (context 5), in one process.  The chain has no exported device-pointer call: it is reached through
        # sea_dnn_enhance_utterances, which times its own stages with device events on its stream (sea_dnn_last_stage_ms):
        # the cochleagram, the splice, every layer (2 M K N FLOP each -> TFLOP/s) and the chain from before the subbands to
        # after the resynthesis; the host call's wall time (upload, launches, download) is given beside them.  On the same
        # list: sea_resynth_utterances alone (with the chain's masks) and sea_hw64_enhance_utterances, wall time.  One warm-up
        # discarded, median of --steps.  The yardstick for a layer is the 122 TFLOP/s of an untuned LDS-tiled GEMM on
        # v_mfma_f32_32x32x2_f32 at 4096^3; this is a first form and there is no target.  The lines also go to
        # profiles/dnn_bench_extra.jsonl.
        import ctypes
        lib = sea.load()
        n = batch.n_utt
        host = batch.data.cpu().numpy()
        lengths = np.asarray(batch.host_lengths, dtype=np.int64)
        xs = [np.ascontiguousarray(host[int(o):int(o) + int(L)]) for o, L in zip(batch.host_offsets, lengths)]
        rows = (lengths - 320) // 160 + 1
        n_rows, samples = int(rows.sum()), int(lengths.sum())
        dims, context = [704, 1024, 1024, 1024, 64], 5
        rng = np.random.default_rng(2025)
        weights = [(rng.standard_normal((dims[l + 1], dims[l])) / np.sqrt(dims[l])).astype(np.float32) for l in range(4)]
        biases = [rng.uniform(-0.5, 0.5, size=dims[l + 1]).astype(np.float32) for l in range(4)]
        model = sea.DnnMask(context, np.full(704, -10.0, np.float32), np.full(704, 0.1, np.float32), weights, biases, [1, 1, 1, 1])
        ptrs = lambda arrs: (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs]) if arrs is not None else None
        lens = (ctypes.c_long * n)(*[int(L) for L in lengths])
        out = [np.zeros(int(L), np.int16) for L in lengths]
        out2 = [np.zeros(int(L), np.int16) for L in lengths]
        masks = [np.zeros((int(r), 64), np.float32) for r in rows]
        workload = (f"the {args.utts}-utterance corpus as 16 kHz int16 utterances: {samples} samples, {n_rows} rows; network "
                    f"{'-'.join(map(str, dims))}, sigmoid, context {context}; median of {args.steps} calls after one warm-up")
        lines = []

        def emit(record):
            lines.append(json.dumps(record))
            print(lines[-1], flush=True)

        STAGES = {"subbands": 0, "cochleagram": 1, "splice": 2, "layer 0": 3, "layer 1": 4, "layer 2": 5, "layer 3": 6, "resynthesis": 11,
                  "chain": 12}
        stage_ms = {k: [] for k in STAGES}
        wall_ms = []
        for i in range(args.steps + 1):
            t0 = time.perf_counter()
            assert lib.sea_dnn_enhance_utterances(model._handle, ptrs(xs), lens, n, 0, ptrs(out), ptrs(masks)) == 0, lib.sea_last_error()
            if i:
                wall_ms.append((time.perf_counter() - t0) * 1e3)
                for k, st in STAGES.items():
                    stage_ms[k].append(float(lib.sea_dnn_last_stage_ms(st)))
        chunks = int(lib.sea_dnn_last_chunks())
        med = lambda t: sorted(t)[len(t) // 2]
        for k in STAGES:
            t = sorted(stage_ms[k])
            rec = {"metric": f"DNN mask estimator: {k}, device events inside sea_dnn_enhance_utterances (ms); a first form, not tuned",
                   "value": med(t), "unit": "ms", "config": {"workload": workload, "ms_sorted": [round(v, 3) for v in t]}, "chunks": chunks}
            if k.startswith("layer"):
                l = int(k.split()[1])
                flop = 2.0 * n_rows * dims[l] * dims[l + 1]
                rec.update(tflops=flop / (med(t) / 1e3) / 1e12, flop=flop, yardstick_tflops=122.0, kernels="sea::dnn_layer_kernel",
                           shape=f"M={n_rows} K={dims[l]} N={dims[l + 1]}")
            if k == "chain":
                rec.update(x_realtime_16k=samples / 16000.0 / (med(t) / 1e3),
                           layers_tflops=sum(2.0 * n_rows * dims[l] * dims[l + 1] for l in range(4)) / (sum(med(stage_ms[f"layer {l}"]) for l in range(4)) / 1e3) / 1e12)
            emit(rec)
        emit({"metric": "DNN mask estimator: sea_dnn_enhance_utterances end to end from host memory, wall time (ms)", "value": med(wall_ms),
              "unit": "ms", "x_realtime_16k": samples / 16000.0 / (med(wall_ms) / 1e3),
              "config": {"workload": workload, "ms_sorted": [round(v, 1) for v in sorted(wall_ms)]}, "chunks": chunks})

        def host_wall(fn):
            t = []
            for i in range(args.steps + 1):
                t0 = time.perf_counter()
                assert fn() == 0, lib.sea_last_error()
                if i:
                    t.append((time.perf_counter() - t0) * 1e3)
            return sorted(t)
        t = host_wall(lambda: lib.sea_resynth_utterances(ptrs(xs), lens, ptrs(masks), 0, ptrs(out2), n))
        assert all(np.array_equal(a, b) for a, b in zip(out, out2)), "the chain's audio is not the resynthesis of its masks"
        emit({"metric": "sea_resynth_utterances alone on the same list with the chain's masks, wall time (ms)", "value": med(t), "unit": "ms",
              "config": {"workload": workload, "ms_sorted": [round(v, 1) for v in t]}, "audio_equals_the_chain": True})
        xf = [x.astype(np.float32) for x in xs]
        audio = [np.zeros(int(L), np.float32) for L in lengths]
        m2 = [np.zeros((int(L) // 160, 64), np.float32) for L in lengths]
        p2 = [np.zeros(int(L) // 160, np.int32) for L in lengths]
        status2 = np.zeros(n, np.int32)
        t = host_wall(lambda: lib.sea_hw64_enhance_utterances(ptrs(xf), lens, n, ptrs(audio), None, ptrs(m2), ptrs(p2),
                                                              status2.ctypes.data_as(ctypes.c_void_p)))
        emit({"metric": "sea_hw64_enhance_utterances (the Hu-Wang estimator and its resynthesis) on the same list, wall time (ms)",
              "value": med(t), "unit": "ms", "config": {"workload": workload, "ms_sorted": [round(v, 1) for v in t]},
              "chunks": int(lib.sea_hw64_enhance_last_chunks())})
        with open(os.path.join(ROOT, "profiles", "dnn_bench_extra.jsonl"), "w") as fh:
            fh.write("\n".join(lines) + "\n")

    if "dnntrain" in what:
        # The DNN mask estimator's trainer: the seeded 704-1024-1024-1024-64 sigmoid network (context 5)
        # on synthetic feature and target rows of the --utts corpus's row count, resident on the device.  Per minibatch size
        # (256, 1024, 4096): one warm-up run, then 5 runs of 200 steps over a seeded order; a run's wall time (the call
        # synchronises its stream) gives steps/s, rows/s and the time of an epoch over the rows; the device time of every stage
        # of a run's last step comes from events on the trainer's stream (sea_dnn_trainer_stage_ms).  Median of the 5 runs, the
        # sorted values beside it.  There is no target: the yardstick written beside each gradient GEMM is the unchanged forward
        # dnn_layer_kernel of the same layer at the same M in the same process (same FLOP count).  The lines also go to
        # profiles/dnntrain_bench_extra.jsonl.
        lengths = np.asarray(batch.host_lengths, dtype=np.int64)
        rows = (lengths - 320) // 160 + 1
        n_rows = int(rows.sum())
        dims, context, n_steps, runs = [704, 1024, 1024, 1024, 64], 5, 200, 5
        rng = np.random.default_rng(2025)
        weights = [(rng.standard_normal((dims[l + 1], dims[l])) / np.sqrt(dims[l])).astype(np.float32) for l in range(4)]
        biases = [rng.uniform(-0.5, 0.5, size=dims[l + 1]).astype(np.float32) for l in range(4)]
        feats = [rng.uniform(0, 27, size=(int(r), 64)).astype(np.float32) for r in rows]
        targets = [rng.uniform(0, 1, size=(int(r), 64)).astype(np.float32) for r in rows]
        shift, scale = sea.DnnMask.normaliser(feats, context)
        model = sea.DnnMask(context, shift, scale, weights, biases, [1, 1, 1, 1])
        trainer = sea.DnnTrainer(model, feats, targets, max_batch=4096)
        med = lambda t: sorted(t)[len(t) // 2]
        lines = []

        def emit(record):
            lines.append(json.dumps(record))
            print(lines[-1], flush=True)

        STAGES = [("gather", 0)] + [(f"forward layer {l}", l) for l in (1, 2, 3, 4)] + [("delta and loss", 9)]
        STAGES += [(f"dgrad layer {l}", 10 + l - 1) for l in (4, 3, 2)] + [(f"wgrad layer {l}", 18 + l - 1) for l in (4, 3, 2, 1)]
        STAGES += [("update", 26), ("step", 27)]
        for B in (256, 1024, 4096):
            workload = (f"{n_rows} synthetic rows ({args.utts} utterances), network {'-'.join(map(str, dims))}, sigmoid, context {context}; "
                        f"minibatch {B}, {n_steps} steps per run, mu 0.9; median of {runs} runs after one warm-up run")
            order = np.random.default_rng(B).integers(0, n_rows, size=n_steps * B)
            stage_ms, wall_s = {k: [] for k, _ in STAGES}, []
            for i in range(runs + 1):
                t0 = time.perf_counter()
                losses = trainer.run(order, B, 1e-3 / B, 0.9)
                if i:
                    wall_s.append(time.perf_counter() - t0)
                    for k, st in STAGES:
                        stage_ms[k].append(trainer.stage_ms(st))
            assert np.all(np.isfinite(losses))
            fwd = {l: 2.0 * B * dims[l - 1] * dims[l] / (med(stage_ms[f"forward layer {l}"]) / 1e3) / 1e12 for l in (1, 2, 3, 4)}
            for k, _ in STAGES:
                t = sorted(stage_ms[k])
                rec = {"metric": f"DNN trainer, minibatch {B}: {k}, device events on the last step of a run (ms); a first form, not tuned",
                       "value": med(t), "unit": "ms", "config": {"workload": workload, "ms_sorted": [round(v, 4) for v in t]}}
                if "layer" in k:
                    l = int(k.split()[-1])
                    flop = 2.0 * B * dims[l - 1] * dims[l]
                    rec.update(tflops=flop / (med(t) / 1e3) / 1e12, flop=flop, shape=f"B={B} K={dims[l - 1]} N={dims[l]}",
                               yardstick_forward_dnn_layer_kernel_same_M_tflops=fwd[l],
                               kernels="sea::dnn_layer_kernel" if k.startswith("forward") else
                               "sea::dnn_dgrad_kernel" if k.startswith("dgrad") else "sea::dnn_wgrad_kernel (with the bias gradient)")
                emit(rec)
            w = sorted(wall_s)
            emit({"metric": f"DNN trainer, minibatch {B}: steps/s over a run of {n_steps} steps, wall time of sea_dnn_trainer_run",
                  "value": n_steps / med(w), "unit": "steps/s", "rows_per_s": n_steps * B / med(w),
                  "epoch_s": n_rows / (n_steps * B / med(w)), "epoch_rows": n_rows, "loss_first": float(losses[0]), "loss_last": float(losses[-1]),
                  "config": {"workload": workload, "run_s_sorted": [round(v, 4) for v in w]}})
        trainer.close()
        with open(os.path.join(ROOT, "profiles", "dnntrain_bench_extra.jsonl"), "w") as fh:
            fh.write("\n".join(lines) + "\n")

    if "score" in what:
        # The objective scores on the --utts corpus batch taken as 16 kHz int16 utterances: the clean
        # audio against itself plus a quarter of the next utterance's samples, hop 160, and two seeded masks of the corpus's row
        # count.  The calls take host memory only and time their own kernels with device events (sea_score_last_stage_ms); the
        # host call's wall time (staging, upload, launches, download) is given beside them.  Bytes read by the frame kernel:
        # 4 per sample (ref and est, int16), by the mask kernel 8 per unit; the share of the HBM peak is written beside each.
        # One warm-up discarded, median of --steps.  A first form; there is no target.  The lines also go to
        # profiles/score_bench_extra.jsonl.
        import ctypes
        lib = sea.load()
        n = batch.n_utt
        host = batch.data.cpu().numpy()
        lengths = np.asarray(batch.host_lengths, dtype=np.int64)
        refs = [np.ascontiguousarray(host[int(o):int(o) + int(L)]) for o, L in zip(batch.host_offsets, lengths)]
        ests = [np.clip(r.astype(np.int32) + np.resize(refs[(u + 1) % n], r.size) // 4, -32768, 32767).astype(np.int16)
                for u, r in enumerate(refs)]
        rows = np.maximum((lengths - 320) // 160 + 1, 0)
        n_rows, samples = int(rows.sum()), int(lengths.sum())
        rng = np.random.default_rng(2026)
        m_est = [rng.uniform(0, 1, size=(int(r), 64)).astype(np.float32) for r in rows]
        m_ideal = [rng.uniform(0, 1, size=(int(r), 64)).astype(np.float32) for r in rows]
        ptrs = lambda arrs: (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        lens = (ctypes.c_long * n)(*[int(L) for L in lengths])
        nr = (ctypes.c_int * n)(*[int(r) for r in rows])
        sums, seg, used, counts = np.zeros((n, 3), np.int64), np.zeros(n, np.float64), np.zeros(n, np.int32), np.zeros((n, 4), np.int64)
        workload = (f"the {args.utts}-utterance corpus as 16 kHz int16 utterances: {samples} samples, {n_rows} frames and mask rows; "
                    f"median of {args.steps} calls after one warm-up")
        med = lambda t: sorted(t)[len(t) // 2]
        lines = []

        def emit(record):
            lines.append(json.dumps(record))
            print(lines[-1], flush=True)

        calls = (("sea_score_utterances", lambda: lib.sea_score_utterances(ptrs(refs), ptrs(ests), lens, n, 160, vp(sums), vp(seg), vp(used), None),
                  (("sea::score_frames_kernel<160>", 0, 4 * samples), ("sea::score_finish_kernel", 1, 4 * n_rows + 96 * (samples // 40320 + n)))),
                 ("sea_mask_score_utterances", lambda: lib.sea_mask_score_utterances(ptrs(m_est), ptrs(m_ideal), nr, n, 0.5, 0.5, vp(counts)),
                  (("sea::mask_score_kernel", 2, 512 * n_rows),)))
        for name, fn, kernels in calls:
            wall, stage = [], {k: [] for k, _, _ in kernels}
            for i in range(args.steps + 1):
                t0 = time.perf_counter()
                assert fn() == 0, lib.sea_last_error()
                if i:
                    wall.append((time.perf_counter() - t0) * 1e3)
                    for k, st, _ in kernels:
                        stage[k].append(float(lib.sea_score_last_stage_ms(st)))
            chunks = int(lib.sea_score_last_chunks())
            for k, _, nbytes in kernels:
                t = sorted(stage[k])
                gbps = nbytes / (med(t) / 1e3) / 1e9
                emit({"metric": f"objective scores: {k}, device events inside {name} (ms); a first form, not tuned", "value": med(t),
                      "unit": "ms", "bytes_read": nbytes, "GBps": gbps, "hbm_peak_GBps": HBM_PEAK_GBPS, "frac_of_hbm_peak": gbps / HBM_PEAK_GBPS,
                      "config": {"workload": workload, "ms_sorted": [round(v, 4) for v in t]}, "chunks": chunks})
            emit({"metric": f"objective scores: {name} from host memory, wall time, PCIe inclusive (ms)", "value": med(wall), "unit": "ms",
                  "bytes_uploaded": sum(b for _, st, b in kernels if st != 1), "x_realtime_16k": samples / 16000.0 / (med(wall) / 1e3),
                  "config": {"workload": workload, "ms_sorted": [round(v, 2) for v in sorted(wall)]}, "chunks": chunks})
        assert int(used.sum()) > 0 and int(counts.sum()) == 64 * n_rows
        with open(os.path.join(ROOT, "profiles", "score_bench_extra.jsonl"), "w") as fh:
            fh.write("\n".join(lines) + "\n")

    if "stoi" in what:
        # STOI on the --utts corpus batch taken as 16 kHz int16 utterances: the clean audio against
        # itself plus a quarter of the next utterance's samples.  The call takes host memory only and times its own kernels with
        # device events (sea_stoi_last_stage_ms); the host call's wall time (staging, upload, launches, download) is given beside
        # them.  The band kernel multiplies the kept frames of both signals [rows][256] by the basis [256][424] on the f32 MFMA:
        # 2 * rows * 256 * 424 flop, beside the DNN forward layer's rate on the same corpus (section 5.21: 60 TFLOP/s at
        # 1024 x 1024, M = 407 816).  One warm-up discarded, median of --steps.  A first form; there is no target.  The lines
        # also go to profiles/stoi_bench_extra.jsonl.
        import ctypes
        lib = sea.load()
        n = batch.n_utt
        host = batch.data.cpu().numpy()
        lengths = np.asarray(batch.host_lengths, dtype=np.int64)
        refs = [np.ascontiguousarray(host[int(o):int(o) + int(L)]) for o, L in zip(batch.host_offsets, lengths)]
        ests = [np.clip(r.astype(np.int32) + np.resize(refs[(u + 1) % n], r.size) // 4, -32768, 32767).astype(np.int16)
                for u, r in enumerate(refs)]
        ptrs = lambda arrs: (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        lens = (ctypes.c_long * n)(*[int(L) for L in lengths])
        ssum, terms, fk = np.zeros(n, np.float64), np.zeros(n, np.int64), np.zeros((n, 2), np.int32)
        samples = int(lengths.sum())
        med = lambda t: sorted(t)[len(t) // 2]
        names = ("sea::stoi_resample_kernel", "sea::stoi_energy_kernel", "sea::stoi_compact_kernel", "sea::stoi_band_kernel",
                 "sea::stoi_segment_kernel", "sea::stoi_finish_kernel")
        wall, stage = [], [[] for _ in names]
        for i in range(args.steps + 1):
            t0 = time.perf_counter()
            assert lib.sea_stoi_utterances(ptrs(refs), ptrs(ests), lens, n, 16000, vp(ssum), vp(terms), vp(fk), None) == 0, lib.sea_last_error()
            if i:
                wall.append((time.perf_counter() - t0) * 1e3)
                for st in range(len(names)):
                    stage[st].append(float(lib.sea_stoi_last_stage_ms(st)))
        chunks = int(lib.sea_stoi_last_chunks())
        frames, kept, n_terms = int(fk[:, 0].sum()), int(fk[:, 1].sum()), int(terms.sum())
        workload = (f"the {args.utts}-utterance corpus as 16 kHz int16 utterances: {samples} samples, {frames} frames at 10 kHz of which "
                    f"{kept} are kept, {n_terms} terms; median of {args.steps} calls after one warm-up")
        lines = []

        def emit(record):
            lines.append(json.dumps(record))
            print(lines[-1], flush=True)

        for st, k in enumerate(names):
            t = sorted(stage[st])
            rec = {"metric": f"STOI: {k}, device events inside sea_stoi_utterances (ms); a first form, not tuned", "value": med(t), "unit": "ms",
                   "config": {"workload": workload, "ms_sorted": [round(v, 4) for v in t]}, "chunks": chunks}
            if k.endswith("band_kernel"):
                flop = 2.0 * (2 * kept) * 256 * 424
                rec.update(flop=flop, TFLOPs=flop / (med(t) / 1e3) / 1e12, dnn_forward_layer_TFLOPs_same_corpus=60.0)
            emit(rec)
        with np.errstate(invalid="ignore"):
            mean_stoi = float(np.nanmean(ssum / terms))
        emit({"metric": "STOI: sea_stoi_utterances from host memory, wall time, PCIe inclusive (ms)", "value": med(wall), "unit": "ms",
              "bytes_uploaded": 4 * samples, "x_realtime_16k": samples / 16000.0 / (med(wall) / 1e3), "mean_stoi": mean_stoi,
              "config": {"workload": workload, "ms_sorted": [round(v, 2) for v in sorted(wall)]}, "chunks": chunks})
        assert n_terms > 0 and 0.0 < mean_stoi < 1.0
        with open(os.path.join(ROOT, "profiles", "stoi_bench_extra.jsonl"), "w") as fh:
            fh.write("\n".join(lines) + "\n")

    if "rfft" in what:
        n = 1 << 18
        x = torch.randn(n, 256, device=dev)
        wall, ker = timed(lambda: sea.rfft_batch(x), args.steps)
        alg = n * 2048
        print(json.dumps({"metric": "rfft256 frames/sec", "value": n / wall, "unit": "frames/s", "ms_per_step": wall * 1e3,
                          "config": {"workload": f"{n} frames of 256 floats"},
                          "roofline": {"bound": "hbm", "kernel": "sea::rfft256_kernel", "achieved": alg / ker / 1e9,
                                       "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": alg / ker / 1e9 / HBM_PEAK_GBPS,
                                       "avg_step_ms": ker * 1e3}}), flush=True)


if __name__ == "__main__":
    main()
