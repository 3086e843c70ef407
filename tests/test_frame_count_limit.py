"""PackedBatch.layout refuses an utterance whose frame count does not fit the NoiseSup kernels' 32-bit frame counters
(the C entry points only see device pointers to the lengths and cannot; the kernel itself would cut such a length)."""
import numpy as np
import pytest


def test_layout_refuses_2_31_frames():
    from speech_enhancement_amd import engine
    lim = engine.MAX_FRAMES_PER_UTTERANCE
    assert lim == 2 ** 31 - 17          # kMaxFrames of ns_pipe6_kernel.hip
    with pytest.raises(ValueError, match="frames"):
        engine.PackedBatch.layout([800, 80 * lim])
    with pytest.raises(ValueError, match="frames"):
        engine.PackedBatch.layout([80 * 2 ** 31 + 5])


def test_layout_accepts_the_longest_countable_utterance():
    from speech_enhancement_amd import engine
    lim = engine.MAX_FRAMES_PER_UTTERANCE
    offsets, total, order = engine.PackedBatch.layout([80 * (lim - 1) + 79, 160])
    assert offsets.dtype == np.int64 and int(offsets[1]) == (80 * (lim - 1) + 79 + 7) // 8 * 8
    assert total == int(offsets[1]) + 160 and list(order) == [0, 1]
