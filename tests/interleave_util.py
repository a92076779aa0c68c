"""Interleaved-frame helpers shared by the interleaved tests and the fixture generator: numpy
(de)interleaving between frames [nframes, len + nroots, depth] (symbol s of codeword j of frame f at
[f, s, j]; include/ezrs.h, "Interleaved frames") and codeword rows [nframes * depth, len + nroots]
in frame-major order k = f * depth + j."""
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "interleaved_ccsds.npz")


def deinterleave(frames):
    """[F, S, D] frames -> [F * D, S] rows (a copy)."""
    F, S, D = frames.shape
    return np.ascontiguousarray(frames.transpose(0, 2, 1)).reshape(F * D, S)


def interleave(rows, nframes, depth):
    """[F * D, S] rows -> [F, S, D] frames (a copy)."""
    S = rows.shape[1]
    return np.ascontiguousarray(rows.reshape(nframes, depth, S).transpose(0, 2, 1))


def frame_view(buf, nframes, nsym, depth, frame_pitch, sym_stride, offset=0):
    """Writable [F, S, D] view of the frames laid out in the flat numpy buffer `buf`."""
    it = buf.itemsize
    return np.lib.stride_tricks.as_strided(buf[offset:], (nframes, nsym, depth),
                                           (frame_pitch * it, sym_stride * it, it))


def load_fixture():
    """The reference-pinned CCSDS cases of tests/golden/interleaved_ccsds.npz as a list of dicts."""
    z = np.load(FIXTURE)
    out = []
    for i in range(int(z["ncases"][0])):
        pre = f"c{i}_"
        out.append({k[len(pre):]: z[k] for k in z.files if k.startswith(pre)})
    return out
