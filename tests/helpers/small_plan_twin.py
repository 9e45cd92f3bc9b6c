"""The launch decisions of the one-compute-unit k x k stage as they stood BEFORE they were collected in
hippyflow_amd/csrc/hfmi_small_plan.h: the ``if`` ladders of the seven launchers of commit 8f8aa05 restated literally -- launch_chol_inv
(hfmi_small.hip:836), launch_chol_mfma (hfmi_chol.hip:532), launch_jacobi_svd (hfmi_small.hip:1614), launch_jacobi_eig
(hfmi_small.hip:1640), launch_sym_eig (hfmi_small.hip:1718), launch_dc_eig (hfmi_eig_dc.hip:1064), launch_lu_solve
(hfmi_small.hip:1943); one comment per branch names the line it restates.  Each function returns the record of
``hfmi_small_plan_predict`` (include/hfmi.h) for what that launcher did; tests/test_small_plan_cpu.py compares word for word."""

CHOL, EIGH, SVD, LU = 0, 1, 2, 3                     # HFMI_SMALL_PLAN_*
KNOB_WORDS, PLAN_WORDS = 12, 84
# enum small_family
(SF_NONE, SF_CHOL_MFMA, SF_CHOL_REG, SF_CHOL_TILE, SF_CHOL_BIG, SF_CHOL_INV, SF_JACOBI_EIG, SF_JACOBI_EIG_DB, SF_JACOBI_SVD,
 SF_JACOBI_VECTORS, SF_JACOBI_VECTORS_WAVE, SF_TRIDIAG, SF_DC, SF_DC_TOP, SF_DC_BACK, SF_LU) = range(16)
REFUSE_RANGE, REFUSE_INSTANCE = 1, 2
# words of the record
(REFUSE, NLAUNCH, WS_BYTES, NREGIONS, ROUTE, USE_LDS, N_EVEN, NB, LDQ, LEVELS, SPLIT_TOP, DC_BITS) = range(12)
LAUNCH0, LAUNCH_WORDS, MAX_LAUNCHES = 12, 9, 4
(L_FAMILY, L_T0, L_T1, L_T2, L_T3, L_THREADS, L_GRID, L_LDS, L_RAISE) = range(9)
REGION0, MAX_REGIONS = 48, 12
KNOB0 = 72

KNOB_NAMES = ("small_threads", "chol_env", "chol_generic", "chol_tile", "jacobi_db", "jacobi_replay_lds", "eig_env", "tri_waves",
              "dc_split_top", "dc_timing", "chol_key", "eig_key")
DEFAULT_KNOBS = dict(small_threads=1024, chol_env=0, chol_generic=0, chol_tile=1, jacobi_db=1, jacobi_replay_lds=0, eig_env=0,
                     tri_waves=8, dc_split_top=1, dc_timing=0, chol_key=-1, eig_key=-1)

SM_MAXK = 256
CHOL_REG_THREADS = 512                # hfmi_small.hip:278
JAC_MAX_SWEEPS = 40                   # hfmi_small.hip:979
DC_THREADS, DC_MAXN = 1024, 256       # hfmi_eig_dc.hip:32, :34
CM_SCR = 4 * 16 * 17                  # hfmi_chol.hip:92
LU_THREADS = 1024                     # hfmi_small.hip:1750
LU_BOOK_BYTES = (64 + 64 + 256 + 128) * 8   # :1751
LU_LDS_BYTES = 163840                 # :1752


def knobs(**changed):
    kn = dict(DEFAULT_KNOBS)
    for name in changed:
        assert name in kn, name
    kn.update(changed)
    return kn


def knob_words(kn):
    return [kn[name] for name in KNOB_NAMES]


class Record:
    def __init__(self, kn):
        self.w = [0] * PLAN_WORDS
        self.w[KNOB0:KNOB0 + KNOB_WORDS] = knob_words(kn)

    def launch(self, family, t, threads, grid, lds, raised):
        i = self.w[NLAUNCH]
        self.w[NLAUNCH] += 1
        t = list(t) + [0] * (4 - len(t))
        self.w[LAUNCH0 + LAUNCH_WORDS * i:LAUNCH0 + LAUNCH_WORDS * (i + 1)] = [family] + t + [threads, grid, lds, int(raised)]

    def region(self, offset, nbytes):
        i = self.w[NREGIONS]
        self.w[NREGIONS] += 1
        self.w[REGION0 + 2 * i:REGION0 + 2 * i + 2] = [offset, nbytes]


def refused(kn, why):
    r = Record(kn)
    r.w[REFUSE] = why
    return r.w


def chol_tiles(k, trr, tcc):          # hfmi_small.hip:819
    ntr, ntc = (k + trr - 1) // trr, (k + tcc - 1) // tcc
    return sum(1 for I in range(ntr) for J in range(ntc) if J * tcc + tcc - 1 >= I * trr)


def lu_panel_width(m):                # hfmi_small.hip:1753
    avail = (LU_LDS_BYTES - LU_BOOK_BYTES - 64) // 8
    if m * (m | 1) <= avail:
        return m
    return ((avail // m) - 1) & ~15


def parent_chol_mfma(k, kn):          # hfmi_chol.hip:532
    if k < 1 or k > SM_MAXK:                                                  # :534
        return refused(kn, REFUSE_RANGE)
    r = Record(kn)
    nb = (k + 15) // 16                                                       # :536
    if nb <= 5:                                                               # :547
        nw, slots = 8, 2
    elif nb <= 7:                                                             # :548
        nw, slots = 8, 4
    elif nb <= 9:                                                             # :549
        nw, slots = 8, 6
    elif nb <= 12:                                                            # :550
        nw, slots = 8, 10
    else:                                                                     # :551
        nw, slots = 8, 17
    shm = (32 + 5 * 256 + nw * CM_SCR + 2 * nb * 256) * 8                     # :540
    r.launch(SF_CHOL_MFMA, (nw, slots), 64 * nw, 1, shm, True)                # :541 attribute, :542 dim3(1), dim3(64 * NWV)
    r.w[NB] = nb
    return r.w


def parent_chol(k, kn):               # hfmi_small.hip:836
    if k < 1 or k > SM_MAXK:                                                  # :838
        return refused(kn, REFUSE_RANGE)
    # :841-844  g_chol_default: the tuning key if it was ever set (chol_tuning_set, :829), else HFMI_CHOL=tile
    chol_default = kn["chol_key"] if kn["chol_key"] >= 0 else kn["chol_env"]
    if chol_default == 0:                                                     # :845
        return parent_chol_mfma(k, kn)
    r = Record(kn)
    r.w[ROUTE] = 1
    use_lds = 1 if k <= 139 else 0                                            # :846
    r.w[USE_LDS] = use_lds
    shmem = (32 + 3 * 256) * 8 + (k * (k | 1) * 8 if use_lds else 0)          # :847
    chol_generic = kn["chol_generic"]                                         # :849
    if use_lds and not chol_generic:                                          # :850
        ept = (k * (k + 1) // 2 + CHOL_REG_THREADS - 1) // CHOL_REG_THREADS   # :851
        shm = (32 + 4 * 256) * 8 + k * (k | 1) * 8                            # :852
        use_tile = kn["chol_tile"]                                            # :861-865
        if use_tile and k >= 8:                                               # :875
            for a, b in ((1, 2), (2, 2), (2, 3), (3, 3), (3, 4), (4, 4), (4, 5)):    # :876-882
                if chol_tiles(k, a, b) <= CHOL_REG_THREADS:
                    break
            else:                                                             # :883
                a, b = 5, 5
            r.launch(SF_CHOL_TILE, (a, b), CHOL_REG_THREADS, 1, shm, True)    # :868-869
        else:
            for e in (1, 2, 4, 6, 8, 12, 16):                                 # :884-890
                if ept <= e:
                    break
            else:                                                             # :891
                e = 20
            r.launch(SF_CHOL_REG, (e,), CHOL_REG_THREADS, 1, shm, True)       # :855-856
    elif not use_lds and not chol_generic:                                    # :894
        shmb = (32 + 4 * 256) * 8                                             # :896
        for a, b in ((4, 4), (4, 5), (5, 5), (5, 6)):                         # :903-906
            if chol_tiles(k, a, b) <= 1024:
                break
        else:                                                                 # :907
            a, b = 6, 6
        r.launch(SF_CHOL_BIG, (a, b), 1024, 1, shmb, False)                   # :898: no attribute
    else:                                                                     # :909
        r.launch(SF_CHOL_INV, (), kn["small_threads"], 1, shmem, True)        # :910-911
    return r.w


def jacobi_log(r, rounds, n):
    log = rounds * (n - 1) * (n // 2) * 16                                    # sizeof(double2)
    r.w[WS_BYTES] = log + 1024 * 4                                            # hfmi_small.hip:1618 / :1644
    r.region(0, log)                                                          # :1621 / :1647  rotlog
    r.region(log, 1024 * 4)                                                   # :1622 / :1648  perm


def parent_jacobi_svd(k, kn):         # hfmi_small.hip:1614
    if k < 1 or k > SM_MAXK:                                                  # :1615
        return refused(kn, REFUSE_RANGE)
    r = Record(kn)
    use_lds = 1 if k <= 139 else 0                                            # :1616
    n = (k + 1) & ~1                                                          # :1617
    r.w[USE_LDS], r.w[N_EVEN] = use_lds, n
    shmem = (32 + 256 + 132) * 8 + (k * (k | 1) * 8 if use_lds else 0)        # :1623
    r.launch(SF_JACOBI_SVD, (use_lds,), kn["small_threads"], 1, shmem, True)  # :1625-1626 / :1629-1630
    r.launch(SF_JACOBI_VECTORS, (), 128, k, 0, False)                         # :1634
    jacobi_log(r, JAC_MAX_SWEEPS + 1, n)
    return r.w


def parent_jacobi_eig(k, kn):         # hfmi_small.hip:1640
    if k < 1 or k > SM_MAXK:                                                  # :1641
        return refused(kn, REFUSE_RANGE)
    r = Record(kn)
    r.w[ROUTE] = 1
    n = (k + 1) & ~1                                                          # :1642
    np_ = n // 2
    use_lds = 1 if n <= 138 else 0                                            # :1643
    shmem = (32 + 256 + 256) * 8 + (n * n * 8 if use_lds else 0)              # :1649
    threads = kn["small_threads"]                                             # :1650
    cells = ((np_ + 1) >> 1) * (np_ + 1)                                      # :1651
    nb = (cells + threads - 1) // threads                                     # :1652
    r.w[USE_LDS], r.w[N_EVEN], r.w[NB] = use_lds, n, nb
    use_db = kn["jacobi_db"]                                                  # :1665-1669
    nblk = np_ * (np_ + 1) // 2                                               # :1670
    shmem_db = (32 + 512 + 256) * 8 + 8 * nblk * 8                            # :1671
    nb_db = (cells + (threads - 128) - 1) // (threads - 128) if threads > 128 else 99    # :1672
    db_min_blocks = 1 if use_db == 2 else 3                                   # :1675
    if use_db and nb >= db_min_blocks and n <= 138 and np_ <= 128 and threads >= 256 and nb_db <= 3 and shmem_db <= 160 * 1024:   # :1676
        inst = 1 if nb_db <= 1 else 2 if nb_db <= 2 else 3                    # :1684-1686
        r.launch(SF_JACOBI_EIG_DB, (inst,), threads, 1, shmem_db, True)       # :1679-1681
    elif nb <= 1:                                                             # :1688
        r.launch(SF_JACOBI_EIG, (1, use_lds), threads, 1, shmem, True)        # :1655-1657, :1662-1663
    elif nb <= 2:                                                             # :1689
        r.launch(SF_JACOBI_EIG, (2, use_lds), threads, 1, shmem, True)
    elif nb <= 3:                                                             # :1690
        r.launch(SF_JACOBI_EIG, (3, use_lds), threads, 1, shmem, True)
    elif nb <= 9:                                                             # :1691
        r.launch(SF_JACOBI_EIG, (9, use_lds), threads, 1, shmem, True)
    else:                                                                     # :1692  HFMI_FAIL "... not instantiated"
        r.w[REFUSE] = REFUSE_INSTANCE
        return r.w
    if n <= 128 and not kn["jacobi_replay_lds"]:                              # :1697
        r.launch(SF_JACOBI_VECTORS_WAVE, (), 256, (k + 3) // 4, 0, False)     # :1698
    else:
        r.launch(SF_JACOBI_VECTORS, (), 128, k, 0, False)                     # :1701
    jacobi_log(r, JAC_MAX_SWEEPS, n)
    return r.w


def parent_dc_eig(k, kn):             # hfmi_eig_dc.hip:1064
    if k < 1 or k > SM_MAXK:                                                  # :1065
        return refused(kn, REFUSE_RANGE)
    r = Record(kn)
    ldq = (k + 15) // 16 * 16                                                 # :1066
    mat = ldq * ldq                                                           # :1067
    doubles = 3 * DC_MAXN + DC_MAXN * ldq + 3 * mat                           # :1069
    r.w[WS_BYTES] = doubles * 8 + (DC_MAXN + 16) * 4 + 16 * 8 + (3 * DC_MAXN + 16) * 4     # :1071
    dvec = 0                                                                  # :1072
    evec = dvec + DC_MAXN * 8                                                 # :1073
    tauv = evec + DC_MAXN * 8                                                 # :1074
    Vh = tauv + DC_MAXN * 8                                                   # :1075
    Qm = Vh + DC_MAXN * ldq * 8                                               # :1076
    Qt = Qm + mat * 8                                                         # :1077
    Sm = Qt + mat * 8                                                         # :1078
    perm = Sm + mat * 8                                                       # :1079
    sexp = perm + DC_MAXN * 4                                                 # :1080
    ticks = sexp + 16 * 4                                                     # :1081
    top_meta = ticks + 16 * 8                                                 # :1082
    offs = [dvec, evec, tauv, Vh, Qm, Qt, Sm, perm, sexp, ticks, top_meta, r.w[WS_BYTES]]
    for a, b in zip(offs[:-1], offs[1:]):
        r.region(a, b - a)
    tri_waves = kn["tri_waves"]                                               # :1084-1088
    if tri_waves == 4:                                                        # :1092
        for kmax, ri, cj in ((32, 8, 1), (64, 16, 1), (80, 20, 2), (96, 24, 2), (128, 32, 2), (144, 36, 3), (160, 40, 3), (192, 48, 3)):   # :1093-1100
            if k <= kmax:
                break
        else:                                                                 # :1101
            ri, cj = 64, 4
        r.launch(SF_TRIDIAG, (ri, cj, 4, 0), 64 * 4, 1, 0, False)             # :1090
    else:
        for kmax, ri, cj in ((32, 4, 1), (64, 8, 1), (96, 12, 2), (128, 16, 2), (160, 20, 3)):     # :1103-1107
            if k <= kmax:
                r.launch(SF_TRIDIAG, (ri, cj, 8, 0), 64 * 8, 1, 0, False)     # :1090
                break
        else:                                                                 # :1108
            if k <= 192:                                                      # :1119
                ri, cj, lr = 20, 3, 32
            elif k <= 224:                                                    # :1120
                ri, cj, lr = 20, 4, 64
            else:                                                             # :1121
                ri, cj, lr = 24, 4, 64
            r.launch(SF_TRIDIAG, (ri, cj, 8, lr), 512, 1, lr * 64 * cj * 8, True)     # :1115-1117
    levels = 0                                                                # :1129
    while (1 << levels) < k:                                                  # :1130
        levels += 1
    split_top = kn["dc_split_top"]                                            # :1143-1147
    a_split_top = 1 if (split_top and k >= 32) else 0                         # :1148
    r.launch(SF_DC, (8 if k <= 128 else 4,), DC_THREADS, 1, 0, False)         # :1150-1151
    top_from_qt = 0
    if a_split_top:                                                           # :1153
        before = levels - 2 if levels >= 2 else 0                             # :1156
        top_from_qt = before & 1                                              # :1157-1158
        T = (k + 15) // 16                                                    # :1159
        r.launch(SF_DC_TOP, (), 64, T * T + 16, 0, False)                     # :1160
    blocks = (k + 3) // 4                                                     # :1164
    swaps = levels - 1 if levels >= 1 else 0                                  # :1165
    fin_in_qt = swaps & 1                                                     # :1166
    if k <= 80:                                                               # :1169
        el = 5
    elif k <= 96:                                                             # :1170
        el = 6
    elif k <= 128:                                                            # :1171
        el = 8
    elif k <= 144:                                                            # :1172
        el = 9
    elif k <= 192:                                                            # :1173
        el = 12
    else:                                                                     # :1174
        el = 16
    r.launch(SF_DC_BACK, (el,), 64, blocks, 0, False)                         # :1168
    timing = 1 if kn["dc_timing"] else 0                                      # :1177
    r.w[LDQ], r.w[LEVELS], r.w[SPLIT_TOP] = ldq, levels, a_split_top
    r.w[DC_BITS] = top_from_qt | (fin_in_qt << 1) | (timing << 2)
    return r.w


def parent_sym_eig(k, method, kn):    # hfmi_small.hip:1718
    # :1719-1722  g_eig_default: the tuning key if it was ever set (eig_tuning_set, :1711), else HFMI_EIG=jacobi
    eig_default = kn["eig_key"] if kn["eig_key"] >= 0 else kn["eig_env"]
    if method == 1 or eig_default == 1:                                       # :1723
        return parent_jacobi_eig(k, kn)
    return parent_dc_eig(k, kn)                                               # :1724


def parent_lu(m, kn):                 # hfmi_small.hip:1943
    if m < 1 or m > SM_MAXK:                                                  # :1944
        return refused(kn, REFUSE_RANGE)
    r = Record(kn)
    nb = lu_panel_width(m)                                                    # :1945
    shm = LU_BOOK_BYTES + m * (nb | 1) * 8                                    # :1946
    r.launch(SF_LU, (), LU_THREADS, 1, shm, True)                             # :1947-1948
    r.w[NB] = nb
    return r.w


def parent_plan(kind, k, method, kn):
    if kind == CHOL:
        return parent_chol(k, kn)
    if kind == EIGH:
        return parent_sym_eig(k, method, kn)
    if kind == SVD:
        return parent_jacobi_svd(k, kn)
    assert kind == LU
    return parent_lu(k, kn)


def parent_env_knobs(env):
    """the knobs as the parent's function-local statics read them from the environment (each at the line of its ladder)"""
    def flag(name):                                                           # env_flag, hfmi_internal.h:38
        e = env.get(name)
        return 1 if (e is not None and e != "" and e != "0") else 0

    def atoi(text):
        text = text.strip()
        digits = ""
        for i, c in enumerate(text):
            if c.isdigit() or (i == 0 and c in "+-"):
                digits += c
            else:
                break
        return int(digits) if digits not in ("", "+", "-") else 0

    kn = dict(DEFAULT_KNOBS)
    if "HFMI_SMALL_THREADS" in env:                                           # hfmi_small.hip:19-21
        v = atoi(env["HFMI_SMALL_THREADS"])
        kn["small_threads"] = 1024 if (v < 64 or v > 1024 or (v & 63)) else v
    kn["chol_env"] = 1 if env.get("HFMI_CHOL") == "tile" else 0               # :842-843
    kn["chol_generic"] = flag("HFMI_CHOL_GENERIC")                            # :849
    kn["chol_tile"] = 0 if ("HFMI_CHOL_TILE" in env and atoi(env["HFMI_CHOL_TILE"]) == 0) else 1     # :863-864
    kn["jacobi_db"] = atoi(env["HFMI_JACOBI_DB"]) if "HFMI_JACOBI_DB" in env else 1                  # :1667-1668
    kn["jacobi_replay_lds"] = flag("HFMI_JACOBI_REPLAY_LDS")                  # :1696
    kn["eig_env"] = 1 if env.get("HFMI_EIG") == "jacobi" else 0               # :1720-1721
    kn["tri_waves"] = 4 if ("HFMI_TRI_WAVES" in env and atoi(env["HFMI_TRI_WAVES"]) == 4) else 8     # hfmi_eig_dc.hip:1086-1087
    kn["dc_split_top"] = atoi(env["HFMI_DC_SPLIT_TOP"]) if "HFMI_DC_SPLIT_TOP" in env else 1         # :1145-1146
    kn["dc_timing"] = flag("HFMI_DC_TIMING")                                  # :1177
    return kn


if __name__ == "__main__":
    # child of tests/test_small_plan_cpu.py: the knobs this process reads from its environment, before and after the tuning keys
    import ctypes as C
    import json
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from hippyflow_amd import _lib as L

    def own(kind, k, method=0):
        words = (C.c_int64 * PLAN_WORDS)()
        L.call("hfmi_small_plan_predict", kind, k, method, None, words)
        return list(words)

    out = {"before": own(CHOL, 100)[KNOB0:], "chol_route": own(CHOL, 100)[ROUTE], "eig_route": own(EIGH, 100)[ROUTE]}
    keys = json.loads(sys.argv[1]) if len(sys.argv) > 1 else {}
    for key, value in keys.items():
        L.call("hfmi_tuning_set", key.encode(), int(value))
    out.update(after=own(CHOL, 100)[KNOB0:], chol_route_after=own(CHOL, 100)[ROUTE], eig_route_after=own(EIGH, 100)[ROUTE])
    print(json.dumps(out))
