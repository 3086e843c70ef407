#!/usr/bin/env python3
"""tools/host_ceps_ab.py PARENT_LIB -- sea_denoise_ceps_utterances on the 1024-utterance corpus through two builds of the library:
PARENT_LIB (libsea_mi355x.so built from the parent commit in a tree of its own) and this tree's, alternating call by call in one
process on one box, warm; wall clock, median and sorted list of 7 calls each after one warm-up call each.  The two results must
be equal bit for bit.  Prints one JSON line (profiles/cepsslices_bench_extra.jsonl holds one)."""
import ctypes
import json
import os
import sys
import time

import numpy as np

if len(sys.argv) != 2:
    sys.exit(__doc__)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import bench  # noqa: E402  (build_shard)
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
batch = bench.build_shard(1024, 0, dev)
lens = np.asarray(batch.host_lengths)
host = batch.data.cpu().numpy()
utts = [host[o:o + l].copy() for o, l in zip(batch.host_offsets, lens)]
n = len(utts)
libs = {"parent": ctypes.CDLL(os.path.abspath(sys.argv[1])),
        "this tree": ctypes.CDLL(os.path.join(ROOT, "speech_enhancement_amd", "libsea_mi355x.so"))}
for l in libs.values():
    l.sea_denoise_ceps_utterances.restype = ctypes.c_int
    l.sea_last_error.restype = ctypes.c_char_p
    l.sea_host_last_slices.restype = ctypes.c_int
outs = [np.zeros(int(l), np.int16) for l in lens]
ceps = [np.zeros((max(int(l) // 80 - 6, 1), 14), np.float32) for l in lens]
ptr = lambda arrs: (ctypes.c_void_p * n)(*[x.ctypes.data for x in arrs])
pin, pout, pceps = ptr(utts), ptr(outs), ptr(ceps)
plen = (ctypes.c_long * n)(*[int(l) for l in lens])
pnc = (ctypes.c_int * n)()
steps = 7
t = {k: [] for k in libs}
rows, bits = {}, {}
for rep in range(steps + 1):
    for name, l in libs.items():
        t0 = time.perf_counter()
        rc = l.sea_denoise_ceps_utterances(pin, pout, pceps, pnc, plen, n)
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == 0, l.sea_last_error()
        if rep:
            t[name].append(dt)
        else:
            rows[name] = sum(pnc)
            bits[name] = (np.concatenate([c[:k].ravel() for c, k in zip(ceps, pnc)]).view(np.uint32).copy(), np.concatenate(outs).copy())
assert rows["parent"] == rows["this tree"]
assert np.array_equal(bits["parent"][0], bits["this tree"][0]) and np.array_equal(bits["parent"][1], bits["this tree"][1]), "results differ"
res = {"metric": "sea_denoise_ceps_utterances, parent commit | this tree, wall clock ms per call (PCIe inclusive)",
       "config": {"workload": f"the 1024-utterance corpus at 8 kHz, {int((lens // 80).sum())} frames, {rows['parent']} cepstral frames; two "
                              "libraries in one process on one box, calls alternating, median of 7 after one warm-up each; rows and audio "
                              "of the two equal bit for bit",
                  "this_tree_slices": int(libs["this tree"].sea_host_last_slices())}}
for name in libs:
    s = sorted(t[name])
    res["config"][name.replace(" ", "_") + "_ms"] = s[len(s) // 2]
    res["config"][name.replace(" ", "_") + "_ms_sorted"] = [round(v, 3) for v in s]
print(json.dumps(res), flush=True)
