"""Writes tests/golden/seq_model_known.npz: per seed error eps of the host model of the shortened FP64 sequences
(tests/seq_model.py EPS), the operands of tests/hard_rounding.py on which the MODEL misrounds.  The model's seeds are the
correctly rounded reciprocal / reciprocal square root times (1 + eps); what the hardware's seed instructions return is not
measured, so the list says nothing about the device (tests/test_hard_rounding_gpu.py does).  It is pinned so that
tests/test_hard_rounding_cpu.py can assert that nothing outside it fails: the list can only shrink.

    python tests/golden/make_seq_model_known.py
"""
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import seq_model  # noqa: E402

if __name__ == "__main__":
    rec = {}
    for i, eps in enumerate(seq_model.EPS):
        for k, v in seq_model.failing_operands(eps).items():
            if len(v):
                rec[f"{i}|{k}"] = v
                print(f"eps {eps:+.3e}  {k:20s} {len(v)}")
    np.savez_compressed(HERE / "seq_model_known.npz", eps=np.array(seq_model.EPS), **rec)
