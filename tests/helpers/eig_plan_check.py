"""``hfmi_eig_plan_predict`` (include/hfmi.h) over many n at once, and the invariants every plan of the whole-GPU eigensolver
must keep whatever the knobs are.  Used by tests/test_eig_plan_cpu.py, in its own process and in the child interpreters that run
with an HFMI_EIG_* switch set (the switches are read once per process).  As a script: ``python eig_plan_check.py`` checks the
invariants on ``knob_sizes()`` and prints the facts the knob cases assert, as one JSON line."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from hippyflow_amd import _lib as L  # noqa: E402

LDS_PER_BLOCK = 163840        # MI355X: LDS of a workgroup, static + dynamic
DEFL_STATIC_LDS = 4108        # k_dcl_deflate<MODE>: __shared__ int s_scan[1024] + s_any, s_K, s_nrot (hfmi_eig_blocked.hip:793-794)
TRI_B_STATIC_LDS = 64         # k_tri_b: __shared__ double s_part[8] (hfmi_eig_blocked.hip:257)
TRI_U_STATIC_LDS = 96         # k_tri_u: __shared__ double s_red[8], s_bc[4] (hfmi_eig_blocked.hip:519)
NO_ATTRIBUTE_LDS = 65536      # dynamic LDS a kernel gets without hipFuncAttributeMaxDynamicSharedMemorySize

# scalars
(ROUTE, NR, LD, NPAD, WY, NBLK, NPANELS, LF, VLEN, BYTES, TRI_B_ATTR, J_UNB, PANEL_COLS, PANEL_ENDS, MIRRORS, LOWER_UPDATES, TAILS,
 MAX_NTILES, MAX_NPVY, MAX_NB, MAX_NPN, SYM_MIN, UNB_MAX, LEAF_MAX) = range(24)
# instances, and the columns of a walk entry
(TRI_A, TRI_A_SLOTS, TRI_B_4_8, TRI_B_8_8, TRI_B_8_16, TRI_B_8_32, TRI_BS_8, TRI_BS_16, TRI_BS_32, TRI_U_4, TRI_U_8, TRI_U_16,
 TRI_U_20) = range(13)
LAUNCHES, NPN, NPVY, LDS = range(4)
ELEM_BYTES = np.array([8, 4, 1, 40])


def region_names():
    """the names of HFMI_EIG_REGIONS (csrc/hfmi_eig_plan.h), in layout order, with their element letters"""
    with open(os.path.join(ROOT, "hippyflow_amd", "csrc", "hfmi_eig_plan.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(r"#define HFMI_EIG_REGIONS\(X\)((?:[^\n]*\\\n)*[^\n]*)", text)
    return re.findall(r"X\((\w+), ([DIBN]),", m.group(1))


def predict(sizes, nvec=None):
    """the four output arrays of hfmi_eig_plan_predict for every n of sizes: (scalars [N, 24], regions [N, 47, 4], levels [N, 7, 4],
    walk [N, 13, 4])"""
    N = len(sizes)
    S = np.zeros((N, 24), np.int64)
    R = np.zeros((N, len(region_names()), 4), np.int64)
    V = np.zeros((N, 7, 4), np.int64)
    W = np.zeros((N, 13, 4), np.int64)
    p64 = C.POINTER(C.c_int64)
    for i, n in enumerate(sizes):
        L.call("hfmi_eig_plan_predict", int(n), int(n if nvec is None else nvec), LDS_PER_BLOCK, DEFL_STATIC_LDS, S[i].ctypes.data_as(p64),
               R[i].ctypes.data_as(p64), V[i].ctypes.data_as(p64), W[i].ctypes.data_as(p64))
    return S, R, V, W


def check_invariants(sizes, S, R, V, W):
    """every assertion names the n that breaks it"""
    sizes = np.asarray(sizes)

    def holds(cond, what):
        bad = sizes[~np.broadcast_to(cond, sizes.shape)]
        assert bad.size == 0, "%s: n = %s" % (what, bad[:8].tolist())

    names = region_names()
    idx = {name: i for i, (name, _) in enumerate(names)}
    on = S[:, ROUTE] == 1                     # the Jacobi route plans nothing
    sizes, S, R, V, W = sizes[on], S[on], R[on], V[on], W[on]
    elem, count, off, nbytes = R[:, :, 0], R[:, :, 1], R[:, :, 2], R[:, :, 3]
    # ---- workspace
    holds((elem == np.array(["DIBN".index(t) for _, t in names])).all(axis=1), "element types follow the list")
    holds((nbytes == count * ELEM_BYTES[elem]).all(axis=1), "bytes = count x element size")
    holds((off[:, 0] == 0) & (off[:, 1:] >= off[:, :-1] + nbytes[:, :-1]).all(axis=1), "regions ascend without overlap")
    holds(off[:, -1] + nbytes[:, -1] <= S[:, BYTES], "regions end inside the workspace")
    holds(((off % 8 == 0) | (elem != 0)).all(axis=1), "double regions are 8-byte aligned")
    holds(((off % 4 == 0) | (elem != 1)).all(axis=1), "int regions are 4-byte aligned")
    holds(off[:, idx["nodes"]] % 16 == 0, "nodes is 16-byte aligned")
    holds(count[:, idx["pn"]] >= S[:, MAX_NPN], "pn holds the partial norms of every column")
    holds(count[:, idx["pvy"]] >= S[:, MAX_NPVY], "pvy holds the partial sums of every column")
    holds(count[:, idx["nodes"]] >= 2 ** np.maximum(S[:, LF] - 1, 0), "the node records hold the widest merge level")
    for name in ("A", "Vh", "Q1", "Q2", "Qg"):
        holds(count[:, idx[name]] == S[:, LD] * S[:, NPAD], name + " is ld x npad")
    holds(off[:, idx["Q2"]] == off[:, idx["Q1"]] + nbytes[:, idx["Q1"]], "Q1 and Q2 are adjacent (one fill)")
    holds(off[:, idx["rs"]] + nbytes[:, idx["rs"]] - off[:, idx["colbuf"]] == 16 * 8 * S[:, VLEN], "one fill of 16 vectors covers colbuf ... rs")
    # ---- geometry
    holds((S[:, LD] >= S[:, NR]) & (S[:, NR] >= sizes) & (S[:, NR] < sizes + 128) & (S[:, NR] % 128 == 0), "ld >= nr >= n")
    holds(S[:, LD] % 16 == 0, "ld is a multiple of 16")
    holds((S[:, NPAD] % S[:, WY] == 0) & (S[:, NPAD] >= sizes) & ((S[:, WY] == 256) | (S[:, WY] == 512)), "npad is a multiple of WY")
    holds((S[:, NBLK] * S[:, WY] == S[:, NPAD]) & (S[:, NPANELS] * 64 == S[:, NPAD]) & (S[:, VLEN] == S[:, NPAD] + 128), "nblk, npanels, vlen")
    # ---- leaves and merges
    holds(S[:, LF] <= 7, "Lf <= 7")
    holds((sizes + 2 ** S[:, LF] - 1) >> S[:, LF] <= 256, "leaves have at most 256 rows")
    for lv in range(7):
        live = S[:, LF] > lv
        cap, mode, lds, raised = (V[:, lv, q] for q in range(4))
        holds(~live | (cap >= (sizes + 2 ** lv - 1) // 2 ** lv + 1), "cap covers the largest node + 1 (level %d)" % lv)
        holds(~live | (lds == cap * np.array([30, 16, 0])[mode]), "LDS bytes of the MODE (level %d)" % lv)
        holds(~live | (lds <= NO_ATTRIBUTE_LDS) | (raised == 1), "deflate: more than 64 KB only with the attribute raised (level %d)" % lv)
        holds(~live | (lds + DEFL_STATIC_LDS <= LDS_PER_BLOCK), "deflate: dynamic + static LDS fit the workgroup (level %d)" % lv)
        holds(live | (V[:, lv] == 0).all(axis=1), "levels beyond Lf stay empty (level %d)" % lv)
    # ---- tridiagonalisation: what an instance reads of the partial sums
    # k_tri_b<UNR, CB> and k_tri_bs<CB> read pn[l + 64 u], u < CB / 8, l < 64, guarded by npn (hfmi_eig_blocked.hip:290-292, :397-399):
    # 64 CB / 8 partial norms at most -- the bound the 129-norm column of k_tri_bs<16> broke
    for inst, cb in ((TRI_B_4_8, 8), (TRI_B_8_8, 8), (TRI_B_8_16, 16), (TRI_B_8_32, 32), (TRI_BS_8, 8), (TRI_BS_16, 16), (TRI_BS_32, 32)):
        holds(W[:, inst, NPN] <= 64 * cb // 8, "instance %d reads every partial norm it is handed" % inst)
    # k_tri_a<SLOTS> reads pvy[l + 64 u], u < NS = SLOTS ? 33 : 8 (hfmi_eig_blocked.hip:187-190), and <true> adds 8 slots per wave of
    # its 8 waves (:169-174): nb <= 64
    holds(W[:, TRI_A, NPVY] <= 64 * 8, "k_tri_a<false> reads every partial sum of v . y")
    holds(W[:, TRI_A_SLOTS, NPVY] <= 64 * 33, "k_tri_a<true> reads every partial sum of v . y")
    holds(S[:, MAX_NB] <= 64, "k_tri_a<true> adds every slot")
    holds(S[:, MAX_NTILES] == S[:, MAX_NB] * (S[:, MAX_NB] + 1) // 2, "tiles of the lower triangle")
    # k_tri_u<UNR>: its three LDS vectors have L = lds / 24 rows each; a column is L / 2 <= 64 UNR 16-byte loads per wave and
    # L <= 512 (UNR / 4) rows per workgroup (hfmi_eig_blocked.hip:515-517, :535, :542-543)
    for inst, unr in ((TRI_U_4, 4), (TRI_U_8, 8), (TRI_U_16, 16), (TRI_U_20, 20)):
        holds(W[:, inst, LDS] <= 24 * 128 * unr, "k_tri_u<%d> covers its columns" % unr)
        holds(W[:, inst, LDS] <= NO_ATTRIBUTE_LDS, "k_tri_u<%d> has no raised attribute" % unr)
        holds(W[:, inst, LDS] + TRI_U_STATIC_LDS <= LDS_PER_BLOCK, "k_tri_u<%d>: LDS fits" % unr)
    for inst in (TRI_B_4_8, TRI_B_8_8, TRI_B_8_16, TRI_B_8_32):
        holds((W[:, inst, LDS] <= NO_ATTRIBUTE_LDS) | (W[:, inst, LDS] <= S[:, TRI_B_ATTR]), "k_tri_b: more than 64 KB only with the attribute raised")
        holds(W[:, inst, LDS] + TRI_B_STATIC_LDS <= LDS_PER_BLOCK, "k_tri_b: dynamic + static LDS fit the workgroup")
    holds(S[:, TRI_B_ATTR] + TRI_B_STATIC_LDS <= LDS_PER_BLOCK, "k_tri_b: the raised attribute fits the workgroup")
    # ---- the walk adds up
    b_or_bs = W[:, TRI_B_4_8:TRI_BS_32 + 1, LAUNCHES].sum(axis=1)
    holds(b_or_bs == S[:, PANEL_COLS], "one products launch per panel column")
    holds(W[:, TRI_A:TRI_A_SLOTS + 1, LAUNCHES].sum(axis=1) == S[:, PANEL_COLS] + S[:, PANEL_ENDS], "one k_tri_a per column and per panel end")
    tail_cols = W[:, TRI_U_4:TRI_U_20 + 1, LAUNCHES].sum(axis=1)
    holds(np.where(S[:, J_UNB] >= 0, (tail_cols == sizes - S[:, J_UNB]) & (S[:, TAILS] == 0), (tail_cols == 0) & (S[:, TAILS] == 1)),
          "the unblocked tail runs from j_unb to n - 1, or k_tri_tail closes the panels")
    holds(np.where(S[:, J_UNB] >= 0, S[:, PANEL_COLS] == S[:, J_UNB], S[:, PANEL_COLS] == sizes - 2), "every column is reduced once")
    holds((S[:, J_UNB] < 0) | ((S[:, J_UNB] % 64 == 0) & (sizes - S[:, J_UNB] <= S[:, UNB_MAX])), "the tail starts at a panel boundary")
    holds(S[:, MIRRORS] <= S[:, LOWER_UPDATES], "a mirror launch follows lower-cut updates only")
    holds((S[:, LOWER_UPDATES] == 0) == (S[:, MIRRORS] == 0), "lower-cut updates are mirrored back")


def knob_sizes():
    """what a child interpreter sweeps: every size up to 700, a stride beyond, and the neighbourhood of every threshold"""
    near = [n for c in (1024, 2048, 3072, 4096, 4300, 8192, 9920, 16384) for n in range(c - 70, c + 71)]
    return sorted({n for n in list(range(3, 700)) + list(range(700, 16385, 61)) + near + [1500] if 3 <= n <= 16384})


def facts(sizes, S, R, V, W):
    at = {n: i for i, n in enumerate(sizes)}
    blocked = S[:, ROUTE] == 1

    def row(n):
        i = at[n]
        return {"route": int(S[i, ROUTE]), "ld": int(S[i, LD]), "nr": int(S[i, NR]), "WY": int(S[i, WY]), "Lf": int(S[i, LF]),
                "j_unb": int(S[i, J_UNB]), "tails": int(S[i, TAILS]), "launches": W[i, :, LAUNCHES].tolist(),
                "lower_updates": int(S[i, LOWER_UPDATES]), "mirrors": int(S[i, MIRRORS]),
                "knobs": S[i, SYM_MIN:LEAF_MAX + 1].tolist()}

    return {"at": {str(n): row(n) for n in (300, 1500, 4096, 4097, 4300, 8192)},
            "blocked_sizes": [int(np.asarray(sizes)[blocked].min()), int(blocked.sum())] if blocked.any() else [0, 0],
            "jacobi_max": int(np.asarray(sizes)[~blocked].max()) if (~blocked).any() else 0,
            "any_bs": bool(W[:, TRI_BS_8:TRI_BS_32 + 1, LAUNCHES].any()), "any_tail_column": bool(W[:, TRI_U_4:, LAUNCHES].any()),
            "any_lower_update": bool(S[:, LOWER_UPDATES].any()), "any_mirror": bool(S[:, MIRRORS].any()),
            "ld_is_nr": bool((S[blocked, LD] == S[blocked, NR]).all()),
            "max_leaf_rows": int((((np.asarray(sizes) + 2 ** S[:, LF] - 1) >> S[:, LF])[blocked & (S[:, LF] < 7)]).max())}


if __name__ == "__main__":
    sizes = knob_sizes()
    out = predict(sizes)
    check_invariants(sizes, *out)
    print(json.dumps(facts(sizes, *out)))
