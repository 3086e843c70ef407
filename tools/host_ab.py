#!/usr/bin/env python3
"""tools/host_ab.py PARENT_LIB ENTRY -- one host call over time slices on the 1024-utterance corpus through two builds of the
library: PARENT_LIB (libsea_mi355x.so built from the parent commit in a tree of its own) and this tree's, alternating call by call
in one process on one box, warm; wall clock, median and sorted list of 7 calls each after one warm-up call each.  The two results
must be equal bit for bit.  ENTRY is one of

    sea_denoise_utterances              the corpus at 8 kHz, audio
    sea_wb_denoise_utterances           the corpus plus as many wideband signals, read as 16 kHz: low band, high-band and code rows
    sea_features_utterances             8 kHz, feature rows only
    sea_wb_features_utterances          16 kHz, feature rows and the low band
    sea_denoise_ceps_utterances         8 kHz, audio and cepstral rows
    sea_wb_denoise_ceps_utterances      16 kHz, low band and cepstral rows

with the arguments tools/bench_extra.py gives that call.  Prints one JSON line (profiles/hostpipe_one_driver_ab.jsonl holds six).
Run it under a time limit, one run per entry:   timeout -k 10 300 python tools/host_ab.py PARENT_LIB ENTRY
(the process also ends itself after SEA_AB_TIMEOUT seconds, default 280)."""
import ctypes
import json
import os
import signal
import sys
import time

import numpy as np

ENTRIES = ("sea_denoise_utterances", "sea_wb_denoise_utterances", "sea_features_utterances", "sea_wb_features_utterances",
           "sea_denoise_ceps_utterances", "sea_wb_denoise_ceps_utterances")
if len(sys.argv) != 3 or sys.argv[2] not in ENTRIES:
    sys.exit(__doc__)
signal.alarm(int(os.environ.get("SEA_AB_TIMEOUT", "280")))  # no handler: the default action ends the process, also inside a call
entry = sys.argv[2]
wide = entry.startswith("sea_wb_")
hop = 160 if wide else 80
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
import bench  # noqa: E402  (build_shard)
import bench_extra  # noqa: E402  (wb_batch)
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
batch = bench.build_shard(1024, 0, dev)
if wide:
    batch = bench_extra.wb_batch(batch, dev)
lens = np.asarray(batch.host_lengths)
nfr = lens // hop
host = batch.data.cpu().numpy()
utts = [host[o:o + l].copy() for o, l in zip(batch.host_offsets, lens)]
n = len(utts)
libs = {"parent": ctypes.CDLL(os.path.abspath(sys.argv[1])),
        "this tree": ctypes.CDLL(os.path.join(ROOT, "speech_enhancement_amd", "libsea_mi355x.so"))}
for l in libs.values():
    getattr(l, entry).restype = ctypes.c_int
    l.sea_last_error.restype = ctypes.c_char_p
    l.sea_host_last_slices.restype = ctypes.c_int
ptr = lambda arrs: (ctypes.c_void_p * n)(*[x.ctypes.data for x in arrs])
outs = [np.zeros(int(f) * 80 if wide else int(l), np.int16) for f, l in zip(nfr, lens)]   # the audio (16 kHz: the low band)
width, cap = {"denoise_utterances": (0, 0), "features_utterances": (15, 6), "denoise_ceps_utterances": (14, -6)}[entry[7 if wide else 4:]]
rows = [np.zeros((max(int(f) + cap, 1), width), np.float32) for f in nfr]                  # feature or cepstral rows
hps, codes = [np.zeros((int(f), 3), np.float32) for f in nfr], [np.zeros((int(f), 9), np.float32) for f in nfr]
pin, pout, prow, php, pcode = ptr(utts), ptr(outs), ptr(rows), ptr(hps), ptr(codes)
plen = (ctypes.c_long * n)(*[int(l) for l in lens])
pcnt = (ctypes.c_int * n)()
args, results = {
    "sea_denoise_utterances": ((pin, pout, plen, n), lambda: outs),
    "sea_wb_denoise_utterances": ((pin, pout, php, pcode, plen, n), lambda: outs + hps + codes),
    "sea_features_utterances": ((pin, None, prow, pcnt, plen, n), lambda: [r[:k] for r, k in zip(rows, pcnt)]),
    "sea_wb_features_utterances": ((pin, pout, prow, pcnt, plen, n), lambda: outs + [r[:k] for r, k in zip(rows, pcnt)]),
    "sea_denoise_ceps_utterances": ((pin, pout, prow, pcnt, plen, n), lambda: outs + [r[:k] for r, k in zip(rows, pcnt)]),
    "sea_wb_denoise_ceps_utterances": ((pin, pout, prow, pcnt, plen, n), lambda: outs + [r[:k] for r, k in zip(rows, pcnt)]),
}[entry]
steps = 7
t = {k: [] for k in libs}
emitted, bits, slices = {}, {}, {}
for rep in range(steps + 1):
    for name, l in libs.items():
        if not rep:
            for a in outs + rows + hps + codes:  # the warm-up call's results are the ones compared: nothing of the other library's
                a.fill(0)
        t0 = time.perf_counter()
        rc = getattr(l, entry)(*args)
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == 0, l.sea_last_error()
        if rep:
            t[name].append(dt)
        else:
            emitted[name], slices[name] = sum(pcnt), int(l.sea_host_last_slices())
            bits[name] = np.concatenate([a.ravel().view(np.uint8) for a in results()]).copy()
assert emitted["parent"] == emitted["this tree"] and slices["parent"] == slices["this tree"]
assert np.array_equal(bits["parent"], bits["this tree"]), "results differ"
res = {"metric": f"{entry}, parent commit | this tree, wall clock ms per call (PCIe inclusive)",
       "config": {"workload": f"{n} utterances at {hop // 10} kHz, {int(nfr.sum())} frames, {emitted['parent']} rows emitted; two libraries in "
                              "one process on one box, calls alternating, median of 7 after one warm-up each; the results of the two "
                              "equal bit for bit",
                  "slices": slices["this tree"], "result_bytes": int(bits["parent"].size)}}
for name in libs:
    s = sorted(t[name])
    res["config"][name.replace(" ", "_") + "_ms"] = s[len(s) // 2]
    res["config"][name.replace(" ", "_") + "_ms_sorted"] = [round(v, 3) for v in s]
print(json.dumps(res), flush=True)
