#!/bin/bash
# MI355X counterpart of enhancement_extract_subband_linux/deal.sh (and of enhancement_extract_test's fixed-SNR variant):
#   ./enhance_extract_subband <cfg> [--no-subband-wavs] [--seed N | --fixed | --plan FILE]
# noisy WAVs, the 3 x 64 subband WAVs and IRM.sIRM for every id of purewavlist
set -e
cd "$(dirname "$0")/.."
make -s -C speech_enhancement_amd/csrc
make -s -C speech_enhancement_amd/host
echo "built: speech_enhancement_amd/host/bin/enhance_extract_subband   (usage: <binary> <cfg> [--no-subband-wavs] [--seed N | --fixed | --plan FILE])"
