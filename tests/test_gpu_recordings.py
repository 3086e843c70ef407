"""BufferDenoise of long recordings on the GPU (speech_enhancement_amd/recordings.py: the chunks of all recordings as the
utterances of one sea_denoise_utterances call, stitched by the plan's map), bit for bit against the numpy model over the
oracle (tests/recordings_model.py) on the recordings of tests/recordings_cases.py."""
import numpy as np
import pytest

from tests import recordings_cases as C

pytestmark = pytest.mark.gpu


def _same(got, want, what):
    assert len(got) == len(want)
    for r, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == np.int16 and a.shape == b.shape, f"{what}: recording {r}"
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, f"{what}: recording {r} ({a.size} samples): {bad.size} samples differ, first at {bad[0]}"


def test_all_recordings_in_one_call_equal_the_model():
    import speech_enhancement_amd as sea
    res = sea.buffer_denoise_recordings(C.recordings(), chunk=C.CHUNK)
    model = C.stitched(0.0)
    assert res["status"].tolist() == [s for _, _, s in model] and res["status"].tolist().count(1) == 1
    _same(res["audio"], [d for d, _, _ in model], "chunk 1600")
    assert any(a.any() for a in res["audio"])


def test_one_recording_and_other_chunk_lengths():
    import speech_enhancement_amd as sea
    from oracle import oracle as O
    from tests import recordings_model as M
    den = M.oracle_denoise(O.Oracle())
    xs = C.recordings()
    for r in (3, C.LONGEST, 8):
        assert np.array_equal(sea.buffer_denoise(xs[r], chunk=C.CHUNK), C.stitched(0.0)[r][0]), f"recording {r}"
    for chunk in (320, 4000, 16080):
        got = sea.buffer_denoise(xs[C.LONGEST], chunk=chunk)
        assert np.array_equal(got, M.buffer_denoise(xs[C.LONGEST], chunk, den)), f"chunk {chunk}"
    # the chunking changes the result: it is not etsi_denoise's on the whole recording
    whole = sea.buffer_denoise(xs[C.LONGEST], chunk=16080)
    assert not np.array_equal(whole, sea.buffer_denoise(xs[C.LONGEST], chunk=C.CHUNK))
