#!/usr/bin/env python3
"""Generate tests/golden/g13_transposition.npz from the reference's ``utils/shared.py:transposition`` (lines 36-68).

    python tests/golden/gen_transposition_golden.py /path/to/reference/mg/model

The reference is imported read-only, with the inert stubs of gen_golden.py for the third-party modules its ``utils`` package
imports (pretty_midi and so on).  The function is applied to every id of the vocabulary, ``arange(V)[:, None]``, for the offsets
-6 .. 6, with a zero ``controls`` array of ``ControlSeq.dim()`` columns (it indexes ``controls`` even when nobody wants it).
Only the outputs are stored: ``offsets`` int64 [13] and ``table`` int64 [13, V], table[s, v] = the id v becomes at offsets[s]."""
import os
import sys

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))


def main(ref):
    import numpy as np

    sys.path.insert(0, HERE)
    from gen_golden import _stub_modules
    _stub_modules()
    sys.path.insert(0, ref)
    from utils.sequence import ControlSeq, EventSeq
    from utils.shared import transposition

    V = EventSeq.dim()
    offsets = np.arange(-6, 7, dtype=np.int64)
    ids = np.arange(V, dtype=np.int64)[:, None]
    rows = []
    for off in offsets:
        events, _ = transposition(ids.copy(), np.zeros((V, 1, ControlSeq.dim()), dtype=np.float32), int(off))
        rows.append(np.asarray(events, dtype=np.int64).reshape(V))
    np.savez_compressed(os.path.join(HERE, "g13_transposition.npz"), offsets=offsets, table=np.stack(rows))
    print("g13_transposition.npz:", len(offsets), "offsets x", V, "ids")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
