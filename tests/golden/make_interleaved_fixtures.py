"""Generate tests/golden/interleaved_ccsds.npz FROM THE REFERENCE CODEC: RS_CCSDS(255,223) frames of
interleave depth 5 (1275 bytes) and 4 (1020 bytes) for the interleaved entry points
(ezrs_encode_interleaved / ezrs_decode_interleaved, include/ezrs.h).

Run in the build container (where /root/reference exists), after `make -C oracle all`:

    python tests/golden/make_interleaved_fixtures.py

The reference has no interleaving: this script only (de)interleaves with numpy
(tests/interleave_util.py) around the reference's own per-codeword encode / decode calls
(oracle.Ref over oracle/_ref/libezrs_ref.so).  The file holds data only: per case
  depth, enc [F, 255, I] (random data + the reference's parity), bad (0..16 symbol errors per
  codeword, one codeword beyond capacity, erasures on some codewords: a few repeated, a few on
  symbols that are not corrupted), eras [F*I, 32] / neras [F*I] (frame-major codeword order), and
  the reference's result [F*I], corrected frames out [F, 255, I] and positions [F*I, 32].
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))
import oracle as O  # noqa: E402
from interleave_util import FIXTURE, deinterleave, interleave  # noqa: E402

K, NR = 223, 32
CASES = [(5, 3), (4, 2)]          # (depth I, frames)


def main():
    if not O.Ref.available():
        raise SystemExit("oracle/_ref/libezrs_ref.so missing: run `make -C oracle all` first")
    want = O.ccsds_params(K, True)
    idx = next(i for i, _, p in O.Ref.codecs() if p == want)
    rng = np.random.default_rng(0x494C5652)
    arrays = {}
    for ci, (I, F) in enumerate(CASES):
        ncw = F * I
        data = rng.integers(0, 256, (ncw, K)).astype(np.uint8)
        par = np.zeros((ncw, NR), np.uint8)
        O.Ref.encode_batch(idx, data, K, par)
        rows = np.concatenate([data, par], axis=1)
        enc = interleave(rows, F, I)
        bad = rows.copy()
        eras = np.zeros((ncw, NR), np.uint32)
        neras = np.zeros(ncw, np.uint32)
        over = int(rng.integers(0, ncw))
        for k in range(ncw):
            if k == over:
                e, f = NR // 2 + 3, 0
            elif k % 3 == 1:                              # erasures: 2e + f <= NR
                f = int(rng.integers(1, 9))
                dup = f > 2 and k % 2 == 1                # the repeated one's symbol becomes an error
                e = int(rng.integers(0, (NR - f) // 2 + (0 if dup else 1)))
            else:
                e, f = int(rng.integers(0, NR // 2 + 1)), 0
            locs = rng.choice(K + NR, e + f, replace=False)
            vals = rng.integers(1, 256, e + f).astype(np.uint8)
            if f > 1:
                vals[e] = 0                               # an erasure on an uncorrupted symbol
            bad[k, locs] ^= vals
            ep = locs[e:].astype(np.uint32)
            if f > 2 and k % 2 == 1:
                ep[1] = ep[0]                             # a repeated erasure
            eras[k, :f] = ep
            neras[k] = f
        d, p = bad[:, :K].copy(), bad[:, K:].copy()
        pos = np.zeros((ncw, NR), np.uint32)
        res = O.Ref.decode_batch(idx, d, K, p, eras, neras, pos)
        out = interleave(np.concatenate([d, p], axis=1), F, I)
        assert np.array_equal(deinterleave(enc), rows)
        pre = f"c{ci}_"
        for name, v in (("depth", np.array([I])), ("enc", enc), ("bad", interleave(bad, F, I)),
                        ("eras", eras), ("neras", neras), ("result", res), ("out", out),
                        ("positions", pos)):
            arrays[pre + name] = v
        print(f"case {ci}: I = {I}, {F} frames: results {res.tolist()}")
    arrays["ncases"] = np.array([len(CASES)])
    np.savez_compressed(FIXTURE, **arrays)
    print(os.path.relpath(FIXTURE), "written,", os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    main()
