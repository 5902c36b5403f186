"""Shared by the packed-filter tests: the fragment-order pack of include/sequitr_hip.h ("Fragment-order filter pack") restated in
numpy from its definition, and the 64-channel-block plan a packed case must reach.

    wp[((((cb * Cin/16 + c) * 9 + tap) * 4 + s) * 64 + 16 kk + li) * 4 + nb] = w[tap][16 c + 4 s + kk][64 cb + 16 nb + li]
"""
import numpy as np

from tests import f32_walk_cases as wc


def pack_index(Cin, Cout):
    """flat index into w.reshape(-1) of every element of the pack, in pack order (int64, 9 Cin Cout entries)"""
    nchunk, cblocks = Cin // 16, Cout // 64
    cb, c, tap, s, kk, li, nb = np.meshgrid(np.arange(cblocks), np.arange(nchunk), np.arange(9), np.arange(4), np.arange(4),
                                            np.arange(16), np.arange(4), indexing="ij")
    # the pack's axes in storage order: cb, c, tap, s, lane = (kk, li), nb
    src = (tap * Cin + 16 * c + 4 * s + kk) * Cout + 64 * cb + 16 * nb + li
    return src.reshape(-1).astype(np.int64)


def pack_numpy(w):
    """the pack of a (3,3,Cin,Cout) float32 filter: a gather, so every bit pattern survives"""
    K, K2, Cin, Cout = w.shape
    assert (K, K2) == (3, 3) and Cin % 16 == 0 and Cout % 64 == 0
    return np.ascontiguousarray(w).reshape(-1)[pack_index(Cin, Cout)]


def on_64_blocks(form, N, H, W, Cin, Cout, act="relu"):
    """(taken, walk): does the tile-walk plan put the call on 64-channel blocks of the generic kernel -- ntiles x Cout / 64 >= 512 --
    the only plan a pack is read at (sq_conv_walk_plan; wc.PLAIN or wc.POOL)"""
    p = wc.walk(form, N, H, W, Cin, Cout, 3, act)
    return (p["kernel"] == wc.V2 and Cout % 64 == 0 and p["cblocks"] == Cout // 64 and p["items"] * p["cblocks"] >= 512), p
