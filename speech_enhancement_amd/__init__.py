"""speech_enhancement_amd -- MI355X (gfx950) engine for the per-frame noise-suppression hot path of
guokiddo1/speech_enhancement: etsi/ two-stage Wiener NoiseSup + rfft + CompCeps and the
resyth_64sub_{ori,IBM} 64-band gammatone resynthesis, as hand-written HIP kernels behind the
reference's own C entry points (include/sea_mi355x.h).

Only what that path needs lives here:
  csrc/       HIP kernels, host table builder, the C ABI (libsea_mi355x.so, built in-tree)
  engine.py   host-side mirror of the reference interface + batched HBM-resident forms
  hw25.py     the same for the Hu-Wang mask estimator and its resynthesis on the 25-channel bank
  dnn.py      the DNN mask estimator: cochleagram, feed-forward network, its trainer, the chain from noisy to enhanced audio
  scores.py   objective scores: SNR, SI-SDR, segmental SNR and STOI of enhanced audio; HIT - FA of an estimated mask
  corpus.py   the deterministic synthetic corpus the measurements run on
  shard.py    utterance sharding over the GPUs of a node (LPT / blocks) and the two-scalar job reduction
  host/       plain-C drivers with the reference's command lines (cfg -> list -> WAV in / WAV out) and the
              mask text format; deal/*.sh build them
"""
from . import corpus  # noqa: F401
from ._lib import LIB_PATH, SeaError, load  # noqa: F401
from .engine import (DoCompCeps, MaskBatch, NoiseSup, PackedBatch, afe_features_batch, afe_features_batch_slice,  # noqa: F401
                     afe_slice_state, compceps_batch, features_utterances, ns_denoise_batch_slice, ns_slice_state,
                     compceps_frames, etsi_denoise, gammaToneFilter, irm_target, irm_target_batch, ns_denoise_batch,
                     ns16k_streams_push, ns16k_tables, ns_streams_push, resynth, resynth_batch, resynth_scratch_elems, rfft, rfft_any_batch, rfft_batch, subband_batch, subbband,
                     tables, wb_afe_features_batch, wb_afe_features_batch_slice, wb_afe_slice_state, wb_compceps_batch,
                     wb_denoise, wb_denoise_batch, wb_denoise_batch_slice, wb_denoise_utterances, wb_features_utterances,
                     wb_rows, wb_slice_state, wb_split, wb_tables, cc_slice_state, wb_cc_slice_state, compceps_batch_slice,
                     wb_compceps_batch_slice, denoise_ceps_utterances, wb_denoise_ceps_utterances, addnoise, addnoise_batch,
                     make_trainset, snr_lin, trainset_batch)
from .hw25 import (Hw25Result, hw25_correlogram_batch, hw25_frontend, hw25_frontend_batch, hw25_periphery_batch,  # noqa: F401
                   hw25_split, hw25_tables, Hw25PitchResult, hw25_pitch, hw25_pitch_batch, Hw25AmResult, Hw25MaskResult,
                   hw25_am_batch, hw25_am_tables, hw25_finalseg_batch, hw25_ibm, hw25_ibm_batch, hw25_periphery_gout_batch,
                   Hw25EnhanceResult, hw25_enhance, hw25_enhance_batch, hw25_resynth, hw25_resynth_batch, hw25_resynth_tables)
from .hw64 import (Hw64Result, hw64_correlogram_batch, hw64_frontend, hw64_frontend_batch, hw64_periphery_batch,  # noqa: F401
                   hw64_split, hw64_tables, hw64_workgroups_per_utterance, HW64_STAGE_WORDS, Hw64PitchResult, hw64_pitch,
                   hw64_pitch_batch, hw64_pitch_waves_per_utterance, Hw64AmResult, Hw64MaskResult, hw64_am_batch,
                   hw64_finalseg_batch, hw64_ibm, hw64_ibm_batch, hw64_enhance, hw64_enhance_plan, hw64_enhance_utterances,
                   hw64_resynth, hw64_resynth_tables, hw64_resynth_utterances)
from .dnn import (DnnMask, DnnTrainer, cochleagram, cochleagram_utterances, dnn_enhance_utterances, dnn_forward,  # noqa: F401
                  dnn_last_chunks, dnn_rows)
from .scores import (dnn_score_utterances, mask_scores, score_frames, score_last_chunks, score_utterances,  # noqa: F401
                     stoi_frames, stoi_last_chunks, stoi_utterances)
from .recordings import buffer_denoise, buffer_denoise_recordings, recording_plan, recording_stitch_map  # noqa: F401
