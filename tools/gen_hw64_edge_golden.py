#!/usr/bin/env python3
"""tools/gen_hw64_edge_golden.py -- TEST INFRASTRUCTURE ONLY.

Writes tests/golden/hw64_edge_golden.npz: what THE REFERENCE ITSELF makes of the edge inputs at 16 kHz on the 64-channel bank
(tests/hw64_model.EDGE_INPUTS, tests/hw64_pitch_model.EDGE_HAND_CASES, tests/hw64_am_model.EDGE_HAND_CASES) at every stage:
data only, no reference source.  Runs only where the reference tree exists:

    python tools/gen_hw64_edge_golden.py <reference tree>

The procedure, the assertions and the code are tools/gen_hw25_edge_golden.py's, at the 64-band tools' drivers (HuWang.cpp
copied unmodified to a temporary directory outside the repository and compiled against resyth_64sub_IBM/cpp/HuWang.h) and the
64-band models.  The fixture holds no uint8 array: tests/hw64_model.load_golden () reads every hw64_*.npz and takes one for
the byte planes of a float array.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools import gen_hw25_edge_golden as G  # noqa: E402

if __name__ == "__main__":
    G.main("hw64")
