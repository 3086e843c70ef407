"""Test infrastructure: the caller's-stream contract of the device-pointer entry points (include/sea_mi355x.h, every prototype
whose last parameter is `void *stream`), and the protocol that holds a call to it.

The contract: every launch of the call goes onto the caller's stream, nothing synchronises with the host, the lengths stay on
the device, all scratch is the caller's.  On the default stream a mis-streamed launch cannot be seen, so the protocol moves a
call that an existing test already proves onto a side stream, behind a delay, where an operation that escaped to another stream
cannot come back equal:

 1. on the default stream the module's own helper runs once on the TRUE and once on a DECOY input, with every call of TABLE
    recorded (its arguments, the device allocations behind its pointers, their contents before the first call that sees them);
    the recorded calls are then issued once more on the default stream, on the true run's buffers holding the decoy's
    contents: the warm run whose host-side duration sizes the delay, and after which every buffer holds the decoy's answer;
 2. on a new stream s: (a) a delay kernel; (b) every allocation that the calls may write is filled -- scratch and state blobs
    (the parameters named *scratch*, *inter*, *state*) with 0xFF bytes, every output with what the module's helper had
    put there (its sentinel); (c) every allocation the calls only read receives the true input, the lengths included;
    (d) the recorded C calls, with s's pointer.  The host only enqueues between (a) and the return of (d);
 3. `not s.query()` right after (d): the calls did not wait for the stream;
 4. s.synchronize(), then the module's own helper runs again with its calls of TABLE replaced by copies out of the side-stream
    run's buffers, so that ITS read-back and ITS assertions (oracle, fixture or model; bits, NaNs by position, ratio_tol, guard
    rows) judge the side-stream bytes; the inputs are compared with what went in.

The decoy must differ: after step 1 the buffers hold the decoy's answer, and the module's assertions for the TRUE input must
reject it (`stale_rejected`); a case whose assertions accept the decoy's answer proves nothing and fails.

Which operand is an input is read off the header: a `const` pointer is only read."""
import collections
import contextlib
import ctypes
import functools
import gc
import os
import re
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sea_mi355x.h")

MIN_DELAY_MS, MAX_DELAY_MS, DELAY_FACTOR = 100.0, 1000.0, 20.0
SCRATCH_NAMES = re.compile(r"scratch|inter|state")

Param = collections.namedtuple("Param", "name pointer const")
Row = collections.namedtuple("Row", "prepare expectation")


class ProtocolError(Exception):
    """the harness itself is inconsistent (a replayed call does not line up with its recording): never a verdict on the library"""


# ---- the header ----
def strip_comments(text):
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def stream_prototypes(text=None):
    """{name: [Param, ..]} of every prototype whose last parameter is `void *stream`, comments stripped"""
    if text is None:
        with open(HEADER) as f:
            text = f.read()
    found = {}
    for name, params in re.findall(r"\b(?:int|void|long long)\s+(\w+)\s*\(([^()]*)\)\s*;", strip_comments(text)):
        params = [" ".join(p.split()) for p in params.split(",")]
        if not re.fullmatch(r"void \*\s*stream", params[-1]):
            continue
        found[name] = [Param(re.search(r"(\w+)$", p).group(1), "*" in p, bool(re.match(r"const\b", p))) for p in params]
    return found


# ---- the table: entry point -> (the function of tests/test_gpu_streams.py's RUNS that drives it, what judges it) ----
TABLE = {
    "sea_ns_denoise_batch": Row("ns_short", "oracle: tests.test_gpu_parity.test_ns_batch_vs_oracle, an empty utterance among them"),
    "sea_compceps_batch": Row("ns_chain", "fixture: tests/golden/ns_golden.npz (tests.test_gpu_golden), bits"),
    "sea_rfft256_batch": Row("rfft256", "fixture: tests/golden/rfft_golden.npz, bits"),
    "sea_rfft_batch": Row("rfft_any", "fixture: tests/golden/rfft_sizes_golden.npz, bits"),
    "sea_compceps_frames": Row("compceps_frames", "fixture: tests/golden/compceps_golden.npz"),
    "sea_ns_denoise_batch_slice": Row("ceps_slices_8k", "one launch: tests.test_gpu_ceps_slices._assert_equal"),
    "sea_compceps_batch_slice": Row("ceps_slices_8k", "one launch: tests.test_gpu_ceps_slices._assert_equal"),
    "sea_ns_denoise_batch_fd": Row("afe_chain", "fixture: tests/golden/afe_golden.npz (tests.test_gpu_golden)"),
    "sea_afe_features_batch": Row("afe_chain", "fixture: tests/golden/afe_golden.npz (tests.test_gpu_golden)"),
    "sea_ns_denoise_batch_slice_fd": Row("afe_slices_8k", "one launch: tests.test_gpu_afe_slices._assert_features_equal"),
    "sea_afe_features_batch_slice": Row("afe_slices_8k", "one launch: tests.test_gpu_afe_slices._assert_features_equal"),
    "sea_wb_denoise_batch": Row("wb_chain", "fixture: tests/golden/wb_golden.npz (tests.test_gpu_wb._compare)"),
    "sea_wb_compceps_batch": Row("wb_chain", "fixture: tests/golden/wb_golden.npz (tests.test_gpu_wb._compare)"),
    "sea_wb_denoise_batch_slice": Row("ceps_slices_wb", "one launch: tests.test_gpu_ceps_slices._assert_equal"),
    "sea_wb_compceps_batch_slice": Row("ceps_slices_wb", "one launch: tests.test_gpu_ceps_slices._assert_equal"),
    "sea_wb_denoise_batch_fd": Row("wb_afe_chain", "fixture: tests/golden/wb_afe_golden.npz (tests.test_gpu_wb_afe._compare)"),
    "sea_wb_afe_features_batch": Row("wb_afe_chain", "fixture: tests/golden/wb_afe_golden.npz (tests.test_gpu_wb_afe._compare)"),
    "sea_wb_denoise_batch_slice_fd": Row("afe_slices_wb", "one launch: tests.test_gpu_wb_afe_slices._assert_features_equal"),
    "sea_wb_afe_features_batch_slice": Row("afe_slices_wb", "one launch: tests.test_gpu_wb_afe_slices._assert_features_equal"),
    "sea_resynth64_batch": Row("resynth64", "oracle: the restatement, bits (tests.test_gpu_resynth_model, cases of tests.resynth_model_cases)"),
    "sea_subband64_batch": Row("subband64", "oracle: the restatement, bits (tests.test_gpu_resynth_model, cases of tests.resynth_model_cases)"),
    "sea_irm_target_batch": Row("irm", "model: tests.irm_cases / tests.irm_model, irm_tol"),
    "sea_addnoise_batch": Row("addnoise", "model: tests.addnoise_model, bits"),
    "sea_trainset_batch": Row("trainset", "model: tests.addnoise_model + the separate calls, bits"),
    "sea_hw25_periphery_batch": Row("hw25_two", "fixture: tests/golden/hw25_golden.npz, bits"),
    "sea_hw25_correlogram_batch": Row("hw25_two", "fixture: tests/golden/hw25_golden.npz, bits"),
    "sea_hw25_frontend_batch": Row("hw25_group", "fixture: tests/golden/hw25_golden.npz, bits"),
    "sea_hw25_pitch_batch": Row("hw25_pitch", "fixture: tests/golden/hw25_pitch_golden.npz, bits"),
    "sea_hw25_periphery_gout_batch": Row("hw25_am", "fixture: tests/golden/hw25_am_golden.npz (gOut, bits)"),
    "sea_hw25_am_batch": Row("hw25_am", "fixture: tests/golden/hw25_am_golden.npz, bits and ratio_tol"),
    "sea_hw25_finalseg_batch": Row("hw25_finalseg", "fixture: tests/golden/hw25_am_golden.npz, bits"),
    "sea_hw25_ibm_batch": Row("hw25_ibm", "fixture: tests/golden/hw25_am_golden.npz, createIBM's mask"),
    "sea_hw25_resynth_batch": Row("hw25_resynth", "fixture: tests/golden/hw25_resynth_golden.npz, bits"),
    "sea_hw25_enhance_batch": Row("hw25_enhance", "fixture: tests/golden/hw25_resynth_golden.npz, bits"),
    "sea_hw64_periphery_batch": Row("hw64_two", "fixture: tests/golden/hw64_golden.npz, bits"),
    "sea_hw64_correlogram_batch": Row("hw64_two", "fixture: tests/golden/hw64_golden.npz, bits"),
    "sea_hw64_frontend_batch": Row("hw64_group", "fixture: tests/golden/hw64_golden.npz, bits"),
    "sea_hw64_pitch_batch": Row("hw64_pitch", "fixture: tests/golden/hw64_pitch_golden.npz, bits"),
    "sea_hw64_am_batch": Row("hw64_am", "fixture: tests/golden/hw64_am_golden.npz, bits and ratio_tol"),
    "sea_hw64_finalseg_batch": Row("hw64_finalseg", "fixture: tests/golden/hw64_am_golden.npz, bits"),
    "sea_hw64_ibm_batch": Row("hw64_ibm", "fixture: tests/golden/hw64_am_golden.npz, createIBM's mask"),
    "sea_ns_streams_push": Row("ns_push", "oracle: the reference's DoNoiseSup frame by frame, bits"),
    "sea_ns_streams_push_fd": Row("ns_push_fd", "oracle: the reference's DoNoiseSup and its flags, bits"),
    "sea_ns16k_streams_push": Row("ns16k_push", "oracle: oracle/ns16k_oracle.c (tests.test_gpu_ns16k._compare)"),
}


def rotate(items, k=1):
    """the decoy of a list of utterances: the same utterances, every one at another index -- the same sizes, totals and counts,
    another answer at every index as long as neighbours differ"""
    items = list(items)
    k %= max(len(items), 1)
    return items[k:] + items[:k]


def rotated_index(i, n, k=1):
    """the index in the true list of what sits at index i of rotate(list, k)"""
    return (i + k) % n


# ---- recording ----
class Storage:
    """one device allocation behind a pointer argument: a byte view of all of it, whether any call may write it, the names of
    the parameters that pointed into it and its bytes before the first recorded call that saw it"""

    def __init__(self, view):
        self.view, self.written, self.names, self.snap = view, False, set(), view.clone()

    @property
    def scratch(self):
        return self.written and all(SCRATCH_NAMES.search(n) for n in self.names)


Call = collections.namedtuple("Call", "name args refs")  # refs: per argument None or (storage index, byte offset)


class Record:
    def __init__(self):
        self.calls, self.storages, self._by_ptr, self._allocs = [], [], {}, {}

    def signature(self):
        """what must agree between the true and the decoy run for one to stand in the other's buffers"""
        sig = []
        for c in self.calls:
            scalars = tuple(getattr(a, "value", a) for a, p in zip(c.args, PROTOTYPES[c.name]) if not p.pointer)
            sig.append((c.name, scalars, tuple(c.refs)))
        return sig, [int(s.view.numel()) for s in self.storages]

    def names(self):
        return [c.name for c in self.calls]


PROTOTYPES = stream_prototypes()


def _pointer_value(a):
    if a is None:
        return 0
    if isinstance(a, ctypes.c_void_p):
        return a.value or 0
    return int(a)


def _device_allocations(torch):
    """(address, bytes, storage) of every CUDA tensor alive in this process"""
    seen, out = set(), []
    with warnings.catch_warnings():  # isinstance on a lazy module attribute may warn of its deprecation
        warnings.simplefilter("ignore")
        for o in gc.get_objects():
            try:
                if not isinstance(o, torch.Tensor) or not o.is_cuda:
                    continue
                st = o.untyped_storage()
                a, n = st.data_ptr(), st.nbytes()
            except Exception:
                continue
            if n and a not in seen:
                seen.add(a)
                out.append((a, n, st, o.device))
    return out


def _refs(torch, record, name, args):
    """the storages behind the pointer arguments of one call, registered (and snapshotted) in `record` at first sight"""
    protos = PROTOTYPES[name]
    if len(args) != len(protos):
        raise ProtocolError(f"{name}: {len(args)} arguments, the header has {len(protos)}")
    allocs = None
    refs = []
    for a, p in zip(args, protos):
        v = _pointer_value(a) if p.pointer and p.name != "stream" else 0
        if not v:
            refs.append(None)
            continue
        if v in record._by_ptr:  # seen before: its storage is held, the address cannot have been given to another tensor
            hit = [record._allocs[v]]
        else:
            hit = [x for x in record._allocs.values() if x[0] <= v < x[0] + x[1]]
        if not hit:
            if allocs is None:
                allocs = _device_allocations(torch)
                record._allocs.update({x[0]: x for x in allocs if x[0] not in record._allocs})
            hit = [x for x in allocs if x[0] <= v < x[0] + x[1]]
        if not hit:
            raise ProtocolError(f"{name}: no live device tensor holds argument {p.name} = {v:#x}")
        base, nbytes, st, dev = max(hit, key=lambda x: x[1])
        if base not in record._by_ptr:
            view = torch.empty(0, dtype=torch.uint8, device=dev).set_(st, 0, (nbytes,))
            record._by_ptr[base] = len(record.storages)
            record.storages.append(Storage(view))
        k = record._by_ptr[base]
        s = record.storages[k]
        s.names.add(p.name)
        s.written = s.written or not p.const
        refs.append((k, v - base))
    return refs


@contextlib.contextmanager
def _hooked(make_hook):
    """every entry point of TABLE replaced, on the loaded library object, by make_hook(name, original)"""
    from speech_enhancement_amd import _lib
    lib = _lib.load()
    originals = {name: getattr(lib, name) for name in TABLE}
    try:
        for name, fn in originals.items():
            setattr(lib, name, make_hook(name, fn))
        yield originals
    finally:
        for name, fn in originals.items():
            setattr(lib, name, fn)


def record(run):
    """run() on the default stream with every call of TABLE recorded -> Record"""
    import torch
    rec = Record()

    def make_hook(name, fn):
        def hook(*args):
            if _pointer_value(args[-1]):
                raise ProtocolError(f"{name}: the helper must run on the default stream while it is recorded")
            refs = _refs(torch, rec, name, args)
            rc = fn(*args)
            rec.calls.append(Call(name, args, refs))
            return rc
        return hook

    with _hooked(make_hook):
        run()
    torch.cuda.synchronize()
    if not rec.calls:
        raise ProtocolError("the helper made no call of TABLE")
    return rec


def replay(rec, stream_ptr):
    """the recorded C calls once more, on the recorded buffers, with another stream: enqueues and nothing else"""
    from speech_enhancement_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(stream_ptr)
    for c in rec.calls:
        rc = getattr(lib, c.name)(*c.args[:-1], p)
        if rc != 0:
            raise AssertionError(f"{c.name} returned {rc} on stream {stream_ptr:#x}: {lib.sea_last_error().decode(errors='replace')}")


def substitute(rec, run):
    """run() with its calls of TABLE replaced by copies out of rec's buffers: the helper's own read-back and assertions then
    judge what rec's buffers hold"""
    import torch
    new = Record()
    k = [0]

    def make_hook(name, fn):
        def hook(*args):
            i = k[0]
            k[0] += 1
            if i >= len(rec.calls) or rec.calls[i].name != name:
                raise ProtocolError(f"call {i} of the helper is {name}, the recording has {rec.names()}")
            old = rec.calls[i]
            refs = _refs(torch, new, name, args)
            for r, q, p in zip(refs, old.refs, PROTOTYPES[name]):
                if (r is None) != (q is None):
                    raise ProtocolError(f"{name}: argument {p.name} is null in one run only")
                if r is None or p.const:
                    continue
                dst, src = new.storages[r[0]].view, rec.storages[q[0]].view
                if r[1] != q[1] or dst.numel() != src.numel():
                    raise ProtocolError(f"{name}: argument {p.name} has another size or offset than in the recording")
                dst.copy_(src)
            return 0
        return hook

    with _hooked(make_hook):
        run()
    if k[0] != len(rec.calls):
        raise ProtocolError(f"the helper made {k[0]} calls, the recording has {len(rec.calls)}")


# ---- the delay ----
@functools.lru_cache(maxsize=None)
def _cycles_per_ms():
    """torch.cuda._sleep's argument per millisecond, from one short delay timed with events; None without _sleep"""
    import torch
    if not hasattr(torch.cuda, "_sleep"):
        return None
    probe = 20_000_000
    torch.cuda._sleep(1000)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    torch.cuda._sleep(probe)
    b.record()
    torch.cuda.synchronize()
    return probe / max(a.elapsed_time(b), 1e-3)


@functools.lru_cache(maxsize=None)
def _matmul_delay():
    """the fallback: (a, b, out, matmuls per ms) of a chain of large products"""
    import torch
    a = torch.ones((4096, 4096), device="cuda:0")
    b, out = torch.ones_like(a), torch.empty_like(a)
    torch.mm(a, b, out=out)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(8):
        torch.mm(a, b, out=out)
    e1.record()
    torch.cuda.synchronize()
    return a, b, out, 8 / max(e0.elapsed_time(e1), 1e-3)


def calibrate():
    """once per session, on the default stream, before any side stream has work"""
    if _cycles_per_ms() is None:
        _matmul_delay()


def enqueue_delay(ms):
    """a delay of about `ms` on the current stream; creates no tensor once calibrated"""
    import torch
    per_ms = _cycles_per_ms()
    if per_ms is not None:
        left = int(ms * per_ms)
        while left > 0:  # the argument is a C long on some builds: keep each piece small
            torch.cuda._sleep(min(left, 1_000_000_000))
            left -= 1_000_000_000
        return
    a, b, out, rate = _matmul_delay()
    for _ in range(int(ms * rate) + 1):
        torch.mm(a, b, out=out)


def delay_for(host_ms):
    return min(max(DELAY_FACTOR * host_ms, MIN_DELAY_MS), MAX_DELAY_MS)


# ---- the protocol ----
class Case:
    """one helper `run(variant)` (variant "true" or "decoy"; it launches AND asserts, as the module's test does) through the
    protocol.  prepare / enqueue / verify are separate so that two cases can be pending on two streams at once."""

    def __init__(self, run):
        self.run = run
        self.true = self.decoy = self.stream = None
        self.host_ms = self.delay_ms = None
        self.stale_rejected = self.pending = False

    def load(self, variant):
        """the variant's initial contents into the true run's buffers, on the current stream: (b) and (c) of the protocol"""
        src = {"true": self.true, "decoy": self.decoy}[variant]
        for dst, s in zip(self.true.storages, src.storages):
            if dst.scratch:
                dst.view.fill_(0xFF)
            elif dst.written:
                dst.view.copy_(s.snap)
        for dst, s in zip(self.true.storages, src.storages):
            if not dst.written:
                dst.view.copy_(s.snap)

    def prepare(self):
        import torch
        calibrate()
        self.true = record(lambda: self.run("true"))
        self.decoy = record(lambda: self.run("decoy"))
        if self.true.signature() != self.decoy.signature():
            raise ProtocolError(f"the decoy does not fit the true run's buffers:\n{self.true.signature()}\n{self.decoy.signature()}")
        self.load("decoy")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        replay(self.true, 0)
        self.host_ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        self.delay_ms = delay_for(self.host_ms)
        self.stale_rejected = not self.accepts("true")
        assert self.stale_rejected, "the module's assertions for the true input accept the decoy's answer: the decoy proves nothing"
        return self

    def accepts(self, variant):
        """whether the module's own assertions for `variant` accept what the buffers hold now"""
        try:
            substitute(self.true, lambda: self.run(variant))
        except ProtocolError:
            raise
        except (AssertionError, ValueError, IndexError, KeyError, RuntimeError) as e:
            self.why = repr(e)[:400]
            return False
        return True

    def enqueue(self, stream=None):
        """(a)-(d) on a side stream; the host only enqueues.  Returns whether the stream still had work when (d) returned."""
        import torch
        self.stream = stream or torch.cuda.Stream()
        with torch.cuda.stream(self.stream):
            enqueue_delay(self.delay_ms)
            self.load("true")
            replay(self.true, self.stream.cuda_stream)
        self.pending = not self.stream.query()
        return self.pending

    def verify(self):
        """s.synchronize(), the module's own assertions on the side-stream bytes, the inputs unchanged"""
        import torch
        self.stream.synchronize()
        substitute(self.true, lambda: self.run("true"))
        for i, s in enumerate(self.true.storages):
            if not s.written:
                assert torch.equal(s.view, s.snap), f"input {sorted(s.names)} (allocation {i}) was modified"

    def report(self):
        return f"host {self.host_ms:.3f} ms, delay {self.delay_ms:.0f} ms, {len(self.true.calls)} C calls, " \
               f"{len(self.true.storages)} allocations"
