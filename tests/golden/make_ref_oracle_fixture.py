"""Generates tests/golden/ref_oracle_checks.npz and tests/golden/ref_fuzz_300_424242.npz from the COMPILED REFERENCE
(oracle/_ref/libtsd_ref.so, oracle/Makefile target _ref).  Run in the build container:  python tests/golden/make_ref_oracle_fixture.py
The first holds the inputs of tests/test_cpu_oracle_ref.py and the library's outputs for them, the second the library's digests of
`tools/fuzz_oracle_ref.py 300 424242`: where the library cannot be built, those tests compare the oracle with these files."""
import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import pyoracle as O  # noqa: E402
import tests.test_cpu_oracle_ref as T  # noqa: E402

O.build(with_ref=True)
T.RECORD = {}
for iters in T.CHAIN_ITERS:
    T.test_filter_chain_matches_compiled_reference(iters)
T.test_multiplier_matches_reference_behaviour()
T.test_mathbase_helpers()
with tempfile.TemporaryDirectory() as tmp:
    T.test_text_line_readers_match_compiled_reference(Path(tmp))
np.savez_compressed(T.REF_GOLD, **T.RECORD)
print("wrote", len(T.RECORD), "arrays to", T.REF_GOLD)
subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "fuzz_oracle_ref.py"), "300", "424242",
                       "--write-golden", T.REF_FUZZ_GOLD], cwd=ROOT)
