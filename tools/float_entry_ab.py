#!/usr/bin/env python3
"""tools/float_entry_ab.py PARENT_LIB -- the entry points that take the caller's floats (sea_compceps_frames,
sea_ns_streams_push, sea_ns_streams_push_fd, sea_ns16k_streams_push) through two builds of the library: PARENT_LIB
(libsea_mi355x.so built from the parent commit in a tree of its own) and this tree's, in one process on one box, warm.
Per entry point the two libraries alternate run by run, four runs each after one warm-up run each; a run is CALLS
back-to-back calls between two device events, reported as microseconds per call.  Inputs are finite, so the two results must
be equal bit for bit.  Prints one JSON line per entry point with both medians, both sorted lists, the margin (the larger of
the two min-max spreads) and whether this tree's median is within parent's median + margin.
Run it under a time limit:   timeout -k 10 300 python tools/float_entry_ab.py PARENT_LIB"""
import ctypes
import json
import os
import signal
import sys

import numpy as np

if len(sys.argv) != 2:
    sys.exit(__doc__)
signal.alarm(int(os.environ.get("SEA_AB_TIMEOUT", "280")))  # no handler: the default action ends the process, also inside a call
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

RUNS, CALLS = 4, 10
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
libs = {"parent": ctypes.CDLL(os.path.abspath(sys.argv[1])),
        "this_tree": ctypes.CDLL(os.path.join(ROOT, "speech_enhancement_amd", "libsea_mi355x.so"))}
for l in libs.values():
    l.sea_last_error.restype = ctypes.c_char_p
P = lambda t: ctypes.c_void_p(t.data_ptr())
rng = np.random.default_rng(5)


def stream_signal(B, nfr, hop):
    t = np.arange(nfr * hop)
    x = rng.standard_normal((B, nfr * hop)) * 800 + 2000 * np.sin(t * (8.0 / hop)) * ((t // (20 * hop)) % 2)
    return torch.from_numpy(x.astype(np.float32).reshape(B, nfr, hop)).to(dev)


def entry_compceps():
    n = 131072
    x = torch.from_numpy((rng.standard_normal((n, 201)) * 900).astype(np.float32)).to(dev)
    out = torch.zeros((n, 14), dtype=torch.float32, device=dev)
    return f"{n} frames of 201 floats", [out], lambda l: l.sea_compceps_frames(P(x), P(out), n, None)


def entry_streams(fd):
    B, nfr = 1024, 400
    x = stream_signal(B, nfr, 80)
    out = torch.zeros_like(x)
    prod = torch.zeros((B, nfr), dtype=torch.int32, device=dev)
    flags = torch.zeros((B, nfr), dtype=torch.uint8, device=dev)
    ctr = torch.zeros((B, nfr), dtype=torch.int32, device=dev)
    state = torch.zeros((B, libs["parent"].sea_ns_state_floats()), dtype=torch.float32, device=dev)
    if fd:
        call = lambda l: l.sea_ns_streams_push_fd(P(x), P(out), P(prod), P(flags), P(ctr), P(state), B, nfr, 1, None)
        return f"{B} streams x {nfr} frames of 80", [out, prod, flags, ctr], call
    return f"{B} streams x {nfr} frames of 80", [out, prod], lambda l: l.sea_ns_streams_push(P(x), P(out), P(prod), P(state), B, nfr, 1, None)


def entry_ns16k():
    B, nfr = 1024, 200
    x = stream_signal(B, nfr, 160)
    out = torch.zeros_like(x)
    prod = torch.zeros((B, nfr), dtype=torch.int32, device=dev)
    flags = torch.zeros((B, nfr), dtype=torch.uint8, device=dev)
    ctr = torch.zeros((B, nfr), dtype=torch.int32, device=dev)
    w = torch.zeros((B, nfr, 25), dtype=torch.float32, device=dev)
    state = torch.zeros((B, libs["parent"].sea_ns16k_state_floats()), dtype=torch.float32, device=dev)
    call = lambda l: l.sea_ns16k_streams_push(P(x), P(out), P(prod), P(flags), P(ctr), P(w), P(state), B, nfr, 1, None)
    return f"{B} streams x {nfr} frames of 160", [out, prod, flags, ctr, w], call


def one_run(l, call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(CALLS):
        assert call(l) == 0, l.sea_last_error()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / CALLS


for name, make in (("sea_compceps_frames", entry_compceps), ("sea_ns_streams_push", lambda: entry_streams(False)),
                   ("sea_ns_streams_push_fd", lambda: entry_streams(True)), ("sea_ns16k_streams_push", entry_ns16k)):
    work, results, call = make()
    t, bits = {k: [] for k in libs}, {}
    for rep in range(RUNS + 1):
        for k, l in libs.items():
            if not rep:
                for r in results:
                    r.zero_()
            dt = one_run(l, call)
            if rep:
                t[k].append(dt)
            else:
                bits[k] = [r.cpu().numpy().copy() for r in results]
    same = all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(bits["parent"], bits["this_tree"]))
    s = {k: sorted(v) for k, v in t.items()}
    med = {k: (v[1] + v[2]) / 2 for k, v in s.items()}
    margin = max(v[-1] - v[0] for v in s.values())
    print(json.dumps({"entry": name, "workload": work + f"; {CALLS} calls per run, {RUNS} runs each, alternating; us per call",
                      "parent_us": round(med["parent"], 2), "this_tree_us": round(med["this_tree"], 2),
                      "parent_us_sorted": [round(v, 2) for v in s["parent"]], "this_tree_us_sorted": [round(v, 2) for v in s["this_tree"]],
                      "margin_us": round(margin, 2), "within_margin": bool(med["this_tree"] <= med["parent"] + margin),
                      "results_bit_equal": bool(same)}), flush=True)
    assert same, f"{name}: the two libraries' results differ"
