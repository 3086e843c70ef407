"""Test infrastructure: the launch caps of the grid-stride kernels, read from speech_enhancement_amd/csrc/capi.hip (and, for
the trainer's dnn_sgd_kernel, from dnn_train_capi.hip), and the arithmetic that says how many trips of its loop a workgroup
takes on a given input.

Most kernels outside the NoiseSup frame loop are launched with a capped grid and walk their work in a grid-stride loop; a
test only reaches a loop's second trip when its input is larger than the cap.  The caps are constants of the launch code, so
they are parsed here (a renamed or moved constant fails tests/test_launch_caps_cpu.py, not silently a GPU test) and the GPU
tests take their sizes from the helpers below with the device's CU count.

    entry point                                   work items                               grid
    sea_rfft256_batch                             npair = (nframes + 1) / 2                min (npair, 16 n_cu)
    sea_compceps_frames                           ntile = ceil (nframes / 16)              min (ntile, 8192)
    sea_compceps_batch                            nslot = total / 16 + n_utt               min (nslot, kCcGrid)
    sea_wb_compceps_batch, sea_*compceps_batch_slice   the same                            min (nslot, 16384)
    sea_*afe_features_batch and their _slice forms     nslot = total / 8 + n_utt           min (nslot, kAfeGrid)
    sea_hw25_correlogram_batch                    the frames of one utterance              per_utt = ceil (8 n_cu / n_utt), 1..1024
    sea_dnn_trainer_run (dnn_sgd_kernel, one      npiece = ceil ((N K + N) / 256)          min (npiece, 4096)
      launch per layer; dnn_train_capi.hip)       (256 entries of W, then b, per piece)

Workgroup b of a grid of G takes the items b, b + G, ...: ceil ((work - b) / G) trips.  In the slot kernels utterance u owns
the slots [cum[u] / T + u, cum[u + 1] / T + u + 1) and slot k of an utterance holds its rows kT .. kT + T - 1; a slot past
the utterance's capacity is a spare one that the loop skips, so the helpers count the slots that hold a tile."""
import collections
import os
import re

import numpy as np

CAPI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "speech_enhancement_amd", "csrc", "capi.hip")

Caps = collections.namedtuple("Caps", "cc_grid afe_grid frames_grid wb_cc_grid cc_slice_grid rfft_per_cu hw25_per_cu hw25_clamp "
                                      "cc_tile afe_tile frames_tile")
Trips = collections.namedtuple("Trips", "grid work busiest at_least_2 at_least_3")


def _all(pattern, text, what, count):
    found = re.findall(pattern, text)
    if len(found) != count:
        raise LookupError(f"{what}: expected {count} match(es) of /{pattern}/ in capi.hip, found {len(found)}")
    return found


def _same(values, what):
    flat = {int(v) for item in values for v in (item if isinstance(item, tuple) else (item,))}
    if len(flat) != 1:
        raise LookupError(f"{what}: the definitions disagree: {sorted(flat)}")
    return flat.pop()


def parse(text=None):
    """every cap of the table above from capi.hip's text; LookupError names the constant that is not where it was"""
    if text is None:
        with open(CAPI) as f:
            text = f.read()
    cc_grid = _same(_all(r"constexpr long long kCcGrid = (\d+);", text, "kCcGrid", 1), "kCcGrid")
    _all(r"nslot < kCcGrid \? nslot : kCcGrid", text, "the use of kCcGrid", 1)
    afe_grid = _same(_all(r"constexpr long long kAfeGrid = (\d+);", text, "kAfeGrid", 4), "kAfeGrid")
    _all(r"nslot < kAfeGrid \? nslot : kAfeGrid", text, "the uses of kAfeGrid", 4)
    frames_grid = _same(_all(r"ntile < (\d+) \? ntile : (\d+);", text, "the cap of sea_compceps_frames", 1), "sea_compceps_frames")
    literal = _all(r"nslot < (\d+) \? nslot : (\d+);", text, "the caps of sea_wb_compceps_batch and of the slice cepstra", 2)
    wb_cc_grid, cc_slice_grid = _same(literal[:1], "sea_wb_compceps_batch"), _same(literal[1:], "cc_slice_launch")
    rfft_per_cu = _same(_all(r"npair < (\d+)LL \* c->n_cu \? npair : (\d+)LL \* c->n_cu;", text, "the cap of sea_rfft256_batch", 1),
                        "sea_rfft256_batch")
    hw25_per_cu = _same(_all(r"int per_utt = \((\d+) \* c->n_cu \+ n_utt - 1\) / n_utt;", text, "per_utt of the correlogram", 1),
                        "per_utt")
    hw25_clamp = _same(_all(r"per_utt = per_utt < 1 \? 1 : \(per_utt > (\d+) \? (\d+) : per_utt\);", text,
                            "the clamp of per_utt", 1), "the clamp of per_utt")
    cc_tile = _same(_all(r"nslot = total_frames / (\d+) \+ n_utt;", text, "the 16-frame slot count", 3), "the cepstral tile")
    afe_tile = _same(_all(r"nslot = total_ceps / (\d+) \+ n_utt;", text, "the 8-frame slot count", 4), "the feature chain's tile")
    frames_tile = _same(_all(r"ntile = \(nframes \+ (\d+)\) / (\d+);", text, "the tile count of sea_compceps_frames", 1)[0][1:],
                        "the tile of sea_compceps_frames")
    return Caps(cc_grid, afe_grid, frames_grid, wb_cc_grid, cc_slice_grid, rfft_per_cu, hw25_per_cu, hw25_clamp, cc_tile, afe_tile,
                frames_tile)


def trips(items, grid):
    """items: the indices of the work items that hold work (or their count, for 0 .. count - 1) of a loop
    `for (i = blockIdx.x; i < work; i += grid)`.  Returns Trips: the busiest workgroup's trips and how many workgroups take at
    least two and at least three."""
    items = np.arange(int(items), dtype=np.int64) if np.isscalar(items) else np.asarray(items, dtype=np.int64)
    per = np.bincount(items % grid, minlength=1) if items.size else np.zeros(1, np.int64)
    return Trips(int(grid), int(items.size), int(per.max()), int((per >= 2).sum()), int((per >= 3).sum()))


# ---- dnn_sgd_kernel (dnn_train_capi.hip, dnn_train_kernel.hip) ----
DNN_TRAIN_CAPI = os.path.join(os.path.dirname(CAPI), "dnn_train_capi.hip")
DNN_TRAIN_KERNEL = os.path.join(os.path.dirname(CAPI), "dnn_train_kernel.hip")

SgdCap = collections.namedtuple("SgdCap", "threads grid")


def parse_sgd(capi_text=None, kernel_text=None):
    """the cap of dnn_sgd_kernel's launch -- std::min<long long>((total + 255) / 256, 4096) workgroups of 256 over
    total = N K + N entries -- from dnn_train_capi.hip's text, and the kernel's own stride from dnn_train_kernel.hip's;
    LookupError names what is not where it was"""
    if capi_text is None:
        with open(DNN_TRAIN_CAPI) as f:
            capi_text = f.read()
    if kernel_text is None:
        with open(DNN_TRAIN_KERNEL) as f:
            kernel_text = f.read()

    def one(pattern, text, what, where):
        found = re.findall(pattern, text)
        if len(found) != 1:
            raise LookupError(f"{what}: expected 1 match of /{pattern}/ in {where}, found {len(found)}")
        return found[0]

    one(r"const long long total = \(long long\)sa\.N \* sa\.K \+ sa\.N;", capi_text, "the entry count `total` of dnn_sgd_kernel's launch",
        "dnn_train_capi.hip")
    round_up, per, grid, threads = one(r"hipLaunchKernelGGL\(sea::dnn_sgd_kernel, dim3\(\(unsigned\)std::min<long long>\(\(total \+ (\d+)\) / (\d+), (\d+)\)\), "
                                       r"dim3\((\d+)\)", capi_text, "the launch cap of dnn_sgd_kernel (std::min<long long>((total + 255) / 256, 4096))",
                                       "dnn_train_capi.hip")
    first, stride = one(r"for \(long long i = \(long long\)blockIdx\.x \* (\d+) \+ threadIdx\.x; i < total; i \+= \(long long\)gridDim\.x \* (\d+)\)",
                        kernel_text, "the grid-stride loop of dnn_sgd_kernel", "dnn_train_kernel.hip")
    if not int(round_up) + 1 == int(per) == int(threads) == int(first) == int(stride):
        raise LookupError(f"dnn_sgd_kernel: the piece size disagrees: (total + {round_up}) / {per}, dim3({threads}), "
                          f"blockIdx.x * {first}, gridDim.x * {stride}")
    return SgdCap(int(threads), int(grid))


def sgd_pieces(N, K, cap):
    return (N * K + N + cap.threads - 1) // cap.threads


def sgd_trips(N, K, cap):
    """a layer [N][K] with its N biases: workgroup b takes the 256-entry pieces b, b + grid, ... of the N K + N entries"""
    npiece = sgd_pieces(N, K, cap)
    return trips(npiece, min(npiece, cap.grid))


def sgd_second_trip_entry(cap):
    """the flat index (over W row-major, then b) of the first entry that a workgroup reaches on its second trip"""
    return cap.threads * cap.grid


# ---- sea_rfft256_batch ----
def rfft_pairs(nframes):
    return (nframes + 1) // 2


def rfft_grid(nframes, n_cu, caps):
    return min(rfft_pairs(nframes), caps.rfft_per_cu * n_cu)


def rfft_second_trip_frames(n_cu, caps):
    """the smallest frame count at which one wave takes a second trip"""
    return 2 * caps.rfft_per_cu * n_cu + 1


def rfft_trips(nframes, n_cu, caps):
    return trips(rfft_pairs(nframes), rfft_grid(nframes, n_cu, caps))


# ---- sea_compceps_frames ----
def frames_tiles(nframes, caps):
    return (nframes + caps.frames_tile - 1) // caps.frames_tile


def frames_second_trip_frames(caps):
    return caps.frames_tile * caps.frames_grid + 1


def frames_trips(nframes, caps):
    ntile = frames_tiles(nframes, caps)
    return trips(ntile, min(ntile, caps.frames_grid))


# ---- the slot kernels ----
def slot_count(cum, tile):
    """nslot = total / T + n_utt for the prefix sums of the capacities"""
    cum = np.asarray(cum, dtype=np.int64)
    return int(cum[-1]) // tile + len(cum) - 1


def slot_base(cum, tile):
    """first slot of every utterance (and, last, the slot count)"""
    cum = np.asarray(cum, dtype=np.int64)
    return cum // tile + np.arange(len(cum))


def slot_tiles(cum, tile):
    """(slot index, utterance) of every slot that holds a tile: slot base[u] + k with k T < capacity of u"""
    cum = np.asarray(cum, dtype=np.int64)
    base = slot_base(cum, tile)
    ntile = (np.diff(cum) + tile - 1) // tile
    assert (base[:-1] + ntile <= base[1:]).all(), "an utterance's tiles do not fit its slots"
    utt = np.repeat(np.arange(len(ntile)), ntile)
    first = np.concatenate(([0], np.cumsum(ntile)[:-1]))
    return base[utt] + np.arange(int(ntile.sum())) - first[utt], utt


def slot_second_trip_utterances(grid, total, tile):
    """the smallest utterance count at which a launch over `total` rows has more slots than `grid`"""
    return max(grid + 1 - total // tile, 1)


def slot_trips(cum, tile, grid):
    return trips(slot_tiles(cum, tile)[0], min(slot_count(cum, tile), grid))


def straddles(cum, tile, grid):
    """the utterances that own tiles on both sides of slot index `grid`"""
    slots, utt = slot_tiles(cum, tile)
    return sorted(set(utt[slots < grid].tolist()) & set(utt[slots >= grid].tolist()))


# ---- hw25_correlogram_kernel ----
def hw25_per_utt(n_utt, n_cu, caps):
    return min(max((caps.hw25_per_cu * n_cu + n_utt - 1) // n_utt, 1), caps.hw25_clamp)


def hw25_utterances_for(per_utt, n_cu, caps):
    """the smallest utterance count that gives `per_utt` workgroups per utterance"""
    assert 1 <= per_utt < caps.hw25_clamp
    n = (caps.hw25_per_cu * n_cu + per_utt - 1) // per_utt
    assert hw25_per_utt(n, n_cu, caps) == per_utt and (n == 1 or hw25_per_utt(n - 1, n_cu, caps) > per_utt)
    return n


def hw25_trips(frames, per_utt):
    """frames: the frame count of every utterance; workgroup (u, g) takes ceil ((frames[u] - g) / per_utt) trips"""
    frames = np.asarray(frames, dtype=np.int64)
    per = np.maximum(frames[:, None] - np.arange(per_utt)[None, :] + per_utt - 1, 0) // per_utt
    return Trips(int(per_utt), int(frames.sum()), int(per.max()) if per.size else 0, int((per >= 2).sum()), int((per >= 3).sum()))
