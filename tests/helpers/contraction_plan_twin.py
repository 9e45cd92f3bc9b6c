"""Plain-Python twin of the planners of the three contraction dispatchers of libhfmi (hippyflow_amd/csrc/hfmi_tsgemm_plan.h:
``tn_plan_make`` behind ``tn_panel``, ``nn_plan_make`` behind ``nn_panel``, ``ss_plan_make`` behind ``launch_tsgemm_ss``, and
``reduce_plan_make`` behind ``launch_reduce_partials``).  Given a shape, the tuning knobs and the CU count it returns the plan records
(include/hfmi.h, ``hfmi_plan_read`` / ``hfmi_plan_predict``) the library must append, for nn also the rows handed to the row-panel
hook behind each launch; it also enumerates every instance a dispatcher can reach and generates the case lists of
tests/test_gpu_contraction_instances.py.  Test infrastructure only: a new instance, table entry, rule or knob has to be restated
here, or tests/test_contraction_plan_cpu.py fails.

The cost models are restated operation by operation in the same order, so that the floating-point comparisons fall the same way."""

PLAN_WORDS = 16
TN, NN, NN_RES, SS, SSB, REDUCE = range(6)
KIND_NAMES = ("tn", "nn", "nn_res", "ss", "ssb", "reduce")
FIELDS = {
    TN: ("MT", "NT", "WAVES", "TR", "R4", "grid", "nrb", "nsplit", "direct", "tail_nrb", "tail_nsplit"),
    NN: ("TT", "NT", "WAVES", "R4", "UPPER", "msplit", "full_tiles", "tail_tiles", "grid"),
    NN_RES: ("TT", "NT", "WAVES", "R4", "UPPER", "msplit", "full_tiles", "tail_tiles", "grid"),
    SS: ("TPW", "NQ", "PF", "swap", "same", "nsplit"),
    SSB: ("RT", "CTL", "NQ", "PIPE", "swap", "same", "nsplit"),
    REDUCE: ("route", "RY", "nsplit", "tr", "m", "k"),
}
VEC_LONG, VEC_ROWS, FLAT, PARTIALS = range(4)

DEFAULT_KNOBS = {"waves": 8, "rem4": 1, "ss": 1, "tn_hybrid": 1, "tn_mt": 0, "ss_percu": 2, "ss_blocked": 1, "nn_waves": 0,
                 "nn_tt": 0, "nn_hybrid": 1, "nn_res": 1, "nn_res_tt": 0, "nn_upper": 1, "nn_halve_last": 0, "probe": 0}


def knobs(**kw):
    out = dict(DEFAULT_KNOBS)
    for key, val in kw.items():
        assert key in out, key
        out[key] = val
    return out


def record(kind, *values):
    assert len(values) == len(FIELDS[kind])
    return dict(zip(("kind",) + FIELDS[kind], (KIND_NAMES[kind],) + tuple(int(v) for v in values)))


def decode(words):
    """one record of hfmi_plan_read (PLAN_WORDS ints) -> the dict form used here"""
    kind = int(words[0])
    return record(kind, *words[1:1 + len(FIELDS[kind])])


def round_up(x, m):
    return (x + m - 1) // m * m


def r4_class(cols, nt, rem4):
    rem = cols - (nt - 1) * 16
    return (rem + 3) // 4 if (rem4 and rem <= 12) else 0


# ------------------------------------------------------------------ launch_reduce_partials
def reduce_plan(nsplit, pstride, inner_ld, tr, m, k, rs, cs, ptrs_aligned=True):
    fastn, slown = (m, k) if tr else (k, m)
    cfast, crow = (rs, cs) if tr else (cs, rs)
    aligned = ptrs_aligned and pstride % 2 == 0 and inner_ld % 2 == 0 and crow % 2 == 0
    if cfast == 1 and aligned and fastn * slown >= 65536:
        if not tr and rs == inner_ld:
            return record(REDUCE, VEC_LONG, 0, nsplit, tr, m, k)
        if fastn % 2 == 0:                      # an odd fast extent goes to the scalar kernels below
            return record(REDUCE, VEC_ROWS, 0, nsplit, tr, m, k)
    ry = 4 if nsplit <= 32 else 16
    if not tr and cs == 1 and rs == inner_ld and m * inner_ld >= 65536:
        return record(REDUCE, FLAT, ry, nsplit, 0, m, k)
    return record(REDUCE, PARTIALS, ry, nsplit, tr, m, k)


# ------------------------------------------------------------------ tn_panel
TN_MT_MAX = {4: (0, 8, 8, 8, 8, 6, 5, 4, 4, 3, 3, 2, 2, 2, 2, 2, 2),
             8: (0, 5, 5, 5, 4, 3, 3, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1)}
TN_MT_CASES = (1, 2, 3, 4, 5, 6, 8)            # TN_CASE list of tn_dispatch_mt
TN_LIMIT = {8: 20, 4: 32}                      # MT * NT an instance may have, by WAVES
TN_BK = 32


def tn_mode(nt, kn):
    """workgroup configuration of a panel: 8, 4 or 44"""
    return 4 if nt > 11 else kn["waves"]


def tn_tile(m, k, kn):
    """(mode, waves, mt) of a panel of k columns against m rows"""
    nt = (k + 15) // 16
    mode = tn_mode(nt, kn)
    small4 = mode == 44
    waves = 4 if small4 else mode
    mt = TN_MT_MAX[8 if small4 else waves][nt]
    need = ((m + 15) // 16 + waves - 1) // waves
    mt = min(mt, need)
    if 0 < kn["tn_mt"] < mt:
        mt = kn["tn_mt"]
    if mt == 7:
        mt = 6
    return mode, waves, max(mt, 1)


def tn_plan(m, k, N, kn, num_cus, scale=1.0, beta=0.0, rs=None, cs=1, nsplit_req=0, aliased=False, ptrs_aligned=True):
    """records of one tn_panel call (k <= 256); C is addressed as C[i rs + j cs]; aliased: C is one of the operands; ptrs_aligned:
    C and the workspace are 16-byte aligned"""
    rs = k if rs is None else rs
    assert 1 <= k <= 256
    nt = (k + 15) // 16
    kpad = nt * 16
    Npad = round_up(N, TN_BK)
    tr = rs == 1 and cs != 1
    mode, waves, mt = tn_tile(m, k, kn)
    small4 = mode == 44
    rpb = 16 * waves * mt
    nrb = (m + rpb - 1) // rpb
    mpad = nrb * rpb
    cus = (num_cus if num_cus > 0 else 256) * (2 if small4 else 1)
    stages = Npad // TN_BK
    nsplit = nsplit_req
    if nsplit <= 0:
        best, best_cost = 1, 1e300
        for ns in range(1, 129):
            if ns > 1 and stages // ns < 16:
                break
            blocks = nrb * ns
            rounds = (blocks + cus - 1) // cus
            eff = float(blocks) / float(rounds * cus)
            part_ratio = 2.0 * ns * float(mpad) * kpad / (float(N) * (m + k))
            cost = 1.0 / eff + part_ratio
            if cost < best_cost - 1e-12:
                best_cost, best = cost, ns
        nsplit = best
    can_direct = scale == 1.0 and beta == 0.0 and not aliased
    ns_full = nrb_full = ns_tail = 0
    if nsplit_req <= 0 and kn["tn_hybrid"]:
        ideal = float(nrb) / cus
        part_unit = 2.0 * float(rpb) * kpad / (float(N) * (m + k))
        blocks = nrb * nsplit
        rounds = (blocks + cus - 1) // cus
        best_cost = float(rounds * cus) / float(blocks) + part_unit * nsplit * nrb
        for nsf in (1, 2, 3, 4, 6, 8):
            if nsf > 1 and stages // nsf < 16:
                break
            R = (nrb * nsf) // cus
            if R < 1 or (R * cus) % nsf != 0:
                continue
            nf = R * cus // nsf
            nt_blocks = nrb - nf
            if nt_blocks <= 0:
                continue
            nst = max(1, min(cus // nt_blocks, stages // 16, 128))
            tail_rounds = (nt_blocks * nst + cus - 1) // cus
            time = float(R) / nsf + float(tail_rounds) / nst
            parts = part_unit * ((0.0 if (nsf == 1 and can_direct) else float(nsf) * nf) + float(nst) * nt_blocks)
            cost = time / ideal + parts
            if cost < best_cost - 1e-9:
                best_cost, ns_full, nrb_full, ns_tail = cost, nsf, nf, nst
    r4 = r4_class(k, nt, kn["rem4"]) if waves == 8 else 0
    if mt not in TN_MT_CASES or mt * nt > TN_LIMIT[waves]:
        raise LookupError("tsgemm_tn: no instance for MT=%d NT=%d WAVES=%d" % (mt, nt, waves))
    if ns_full > 0:
        nrb_t = nrb - nrb_full
        mpad_f, mpad_t = nrb_full * rpb, nrb_t * rpb
        chunk_f = round_up((Npad + ns_full - 1) // ns_full, TN_BK)
        ns_full = (Npad + chunk_f - 1) // chunk_f
        chunk_t = round_up((Npad + ns_tail - 1) // ns_tail, TN_BK)
        ns_tail = (Npad + chunk_t - 1) // chunk_t
        direct_f = ns_full == 1 and can_direct
        out = [record(TN, mt, nt, waves, tr, r4, nrb_full * ns_full + nrb_t * ns_tail, nrb_full, ns_full, direct_f, nrb_t, ns_tail)]
        if not direct_f:
            out.append(reduce_plan(ns_full, mpad_f * kpad, mpad_f if tr else kpad, tr, mpad_f, k, rs, cs, ptrs_aligned))
        out.append(reduce_plan(ns_tail, mpad_t * kpad, mpad_t if tr else kpad, tr, m - mpad_f, k, rs, cs, ptrs_aligned))
        return out
    chunk = max(round_up((Npad + nsplit - 1) // nsplit, TN_BK), TN_BK)
    nsplit = max((Npad + chunk - 1) // chunk, 1)
    direct = nsplit == 1 and can_direct
    out = [record(TN, mt, nt, waves, tr, r4, nrb * nsplit, nrb, nsplit, direct, 0, 0)]
    if not direct:
        out.append(reduce_plan(nsplit, mpad * kpad, mpad if tr else kpad, tr, m, k, rs, cs, ptrs_aligned))
    return out


def tn_reachable():
    """every (mode, MT, NT, TR, R4) tn_panel can launch: mode 8 / 4 / 44 (44 runs the WAVES = 4 kernels with the small tiles, two
    workgroups per CU); NT >= 12 takes mode 4 whatever the knob says"""
    out = set()
    for nt in range(1, 17):
        modes = (4,) if nt > 11 else (8, 4, 44)
        for mode in modes:
            for mt in range(1, TN_MT_MAX[4 if mode == 4 else 8][nt] + 1):
                if mt == 7:
                    continue
                for tr in (0, 1):
                    for r4 in ((0, 1, 2, 3) if mode == 8 else (0,)):
                        out.add((mode, mt, nt, tr, r4))
    return out


def tn_instances(reach):
    """the kernel instances <MT, NT, TR, WAVES, R4> behind a set of tn_reachable() entries"""
    return {(mt, nt, tr, 8 if mode == 8 else 4, r4) for mode, mt, nt, tr, r4 in reach}


def tn_compiled():
    """what TN_CASE / TN_NT / TN_R4 instantiate: MT in the case list with MT * NT within the limit, NT 1..16, both waves, both orders"""
    out = set()
    for nt in range(1, 17):
        for waves in (8, 4):
            for mt in TN_MT_CASES:
                if mt * nt <= TN_LIMIT[waves]:
                    for tr in (0, 1):
                        for r4 in ((0, 1, 2, 3) if waves == 8 else (0,)):
                            out.add((mt, nt, tr, waves, r4))
    return out


# ------------------------------------------------------------------ nn_panel
NN_KC = 32
NN_CASE = {1: (8, 8), 2: (8, 8), 3: (8, 5), 4: (8, 4), 5: (6, 3), 6: (5, 2), 7: (4, 2), 8: (4, 2), 9: (3, 2), 10: (3, 1),
           11: (2, 1), 12: (2, 1), 13: (2, 1), 14: (2, 1), 15: (2, 1), 16: (2, 1)}      # NT -> (TT of 4 waves, TT of 8 waves)
NN_RES_TT = {1: 4, 2: 4, 3: 4, 4: 4, 5: 3, 6: 2, 7: 2, 8: 2, 9: 2, 10: 1}                  # NT -> TT of the resident kernel
NN_RES_LDS = 160 * 1024


def nn_cost(num_cus, tile_rows, m, r, N, rate_factor):
    """nn_plan: (modelled time, msplit)"""
    cus = num_cus if num_cus > 0 else 256
    ntiles = (N + tile_rows - 1) // tile_rows
    stages = (m + NN_KC - 1) // NN_KC
    flops = 2.0 * float(ntiles) * tile_rows * float(m) * float(((r + 15) // 16) * 16)
    rate, hbm = 60e12 * rate_factor, 4.0e12
    best, best_t = 1, 1e300
    for ns in range(1, 65):
        if ns > 1 and stages // ns < 8:
            break
        blocks = ntiles * ns
        rounds = (blocks + cus - 1) // cus
        eff = float(blocks) / float(rounds * cus)
        t = flops / (eff * rate) + ((ns + 1.0) * float(N) * r * 8.0 / hbm + 3e-6 if ns > 1 else 0.0)
        if t < best_t - 1e-12:
            best_t, best = t, ns
    return best_t, best


NN_MAX_PANELS = 8


def nn_inst(tt, nt, waves, m, r, N, msplit, kn, num_cus, tail_split=False, hook_panels=0):
    """nn_plan_stream: the launches of the streaming kernel as (record, hook_row0, hook_rows); hook_rows = 0: no hook call.  One
    launch without a row-panel hook; with one (hook_panels > 0) and at least two rounds of whole tiles, whole rounds per panel, the
    last round as two launches of half the tile height where the halve knob, an even TT and the panel budget allow, and the split
    tail tiles with or behind the last panel"""
    r4 = r4_class(r, nt, kn["rem4"])
    tile_rows = 16 * tt * waves
    ntiles = (N + tile_rows - 1) // tile_rows
    cus = num_cus if num_cus > 0 else 256
    full_tiles = 0
    if (msplit > 1 or tail_split) and ntiles >= cus and kn["nn_hybrid"]:
        full_tiles = ntiles // cus * cus
        tail = ntiles - full_tiles
        if tail == 0:
            msplit = 1
        else:
            stages = (m + NN_KC - 1) // NN_KC
            ms = cus // tail
            if ms < 2:
                best, ms = 1.0, 1
                for c in range(2, 9):
                    cost = float((tail * c + cus - 1) // cus) / c + 0.01 * c
                    if cost < best - 1e-9:
                        best, ms = cost, c
            ms = max(min(ms, stages // 4), 1)
            msplit = ms
            if msplit == 1:
                full_tiles = 0
    mchunk = round_up((m + msplit - 1) // msplit, NN_KC)
    msplit = (m + mchunk - 1) // mchunk
    if msplit <= 1:
        full_tiles = 0
    tail_tiles = ntiles - full_tiles

    def rec(t, ms, full, tl):
        return record(NN, t, nt, waves, r4, 0, ms, full, tl, full + tl * ms)

    whole_cnt = full_tiles if msplit > 1 else ntiles
    rounds = whole_cnt // cus
    if hook_panels <= 0 or rounds < 2:
        return [(rec(tt, msplit, full_tiles, tail_tiles), 0, 0)]
    hook_panels = min(hook_panels, NN_MAX_PANELS)
    panels = min(rounds, hook_panels)
    halve = bool(kn["nn_halve_last"]) and tt % 2 == 0 and panels == rounds and panels + 1 <= hook_panels
    out = []
    base = 0
    for p in range(panels):
        last = p == panels - 1
        cnt = whole_cnt - base if last else (rounds // panels + (1 if p < rounds % panels else 0)) * cus
        tl = tail_tiles if (last and msplit > 1) else 0
        row0 = base * tile_rows
        if last and halve:
            cnt_a = cnt // 2
            cnt_b = cnt - cnt_a
            row1 = (base + cnt_a) * tile_rows
            out.append((rec(tt // 2, 1, 2 * cnt_a, 0), row0, row1 - row0))
            out.append((rec(tt // 2, 1, 2 * cnt_b, 0), 0, 0) if tl > 0 else (rec(tt // 2, 1, 2 * cnt_b, 0), row1, N - row1))
            if tl > 0:
                out.append((rec(tt, msplit, 0, tl), row1, N - row1))
        else:
            row1 = N if last else (base + cnt) * tile_rows
            out.append((rec(tt, msplit, cnt, tl if msplit > 1 else 0), row0, row1 - row0))
        base += cnt
    return out


def nn_launches(m, r, N, kn, num_cus, upper_hint=False, hook_panels=0):
    """launches of one nn_panel call (r <= 256) as (record, hook_row0, hook_rows)"""
    assert 1 <= r <= 256
    nt = (r + 15) // 16
    cus = num_cus if num_cus > 0 else 256
    if kn["nn_res"] and nt in NN_RES_TT and N >= 4096:
        sld = nt * 16 + (16 if nt % 2 == 0 else 0)
        if ((m + 3) & ~3) * sld * 8 <= NN_RES_LDS:
            def units(tt):
                tiles = (N + 128 * tt - 1) // (128 * tt)
                return float((tiles + cus - 1) // cus) * tt
            ttv = NN_RES_TT[nt]
            tl = ttv - 1 if ttv > 1 else 1
            lower = kn["nn_res_tt"] == 2 or (kn["nn_res_tt"] == 0 and tl != ttv and units(tl) * 1.05 < units(ttv))
            tt = tl if lower else ttv
            ntiles = (N + 128 * tt - 1) // (128 * tt)
            up = bool(upper_hint and kn["nn_upper"])
            return [(record(NN_RES, tt, nt, 8, r4_class(r, nt, kn["rem4"]), up, 1, ntiles, 0, min(ntiles, cus)), 0, 0)]
    waves = kn["nn_waves"] if kn["nn_waves"] else (8 if nt >= 7 else 4)
    tt4, tt8 = NN_CASE[nt]
    if waves == 8:
        return nn_inst(tt8, nt, 8, m, r, N, nn_cost(num_cus, 128 * tt8, m, r, N, 1.0)[1], kn, num_cus, hook_panels=hook_panels)
    t1 = tt4 - 1 if tt4 > 1 else 1
    t2 = tt4 - 2 if tt4 > 2 else 1
    c0, ms0 = nn_cost(num_cus, 64 * tt4, m, r, N, 1.0)
    c1, ms1 = nn_cost(num_cus, 64 * t1, m, r, N, 0.98) if t1 != tt4 else (1e300, 1)
    c2, ms2 = nn_cost(num_cus, 64 * t2, m, r, N, 0.96) if t2 != t1 else (1e300, 1)
    if kn["nn_hybrid"] and kn["nn_tt"] == 0 and (N + 64 * tt4 - 1) // (64 * tt4) >= cus and m >= 16 * NN_KC:
        return nn_inst(tt4, nt, 4, m, r, N, 1, kn, num_cus, tail_split=True, hook_panels=hook_panels)
    if kn["nn_tt"] == 1:
        tt, ms = tt4, ms0
    elif kn["nn_tt"] == 2:
        tt, ms = t1, ms1
    elif kn["nn_tt"] == 3:
        tt, ms = t2, ms2
    elif c0 <= c1 and c0 <= c2:
        tt, ms = tt4, ms0
    elif c1 <= c2:
        tt, ms = t1, ms1
    else:
        tt, ms = t2, ms2
    return nn_inst(tt, nt, 4, m, r, N, ms, kn, num_cus, hook_panels=hook_panels)


def nn_plan(m, r, N, kn, num_cus, upper_hint=False):
    """record of one nn_panel call (r <= 256) without a row-panel hook"""
    (rec, _, _), = nn_launches(m, r, N, kn, num_cus, upper_hint)
    return rec


def nn_stream_reachable():
    """every streaming instance (TT, NT, WAVES, R4) nn_panel can launch without a row-panel hook"""
    out = set()
    for nt, (tt4, tt8) in NN_CASE.items():
        for r4 in range(4):
            out.add((tt8, nt, 8, r4))
            for tt in {tt4, max(tt4 - 1, 1), max(tt4 - 2, 1)}:
                out.add((tt, nt, 4, r4))
    return out


def nn_res_fits(m, nt):
    sld = nt * 16 + (16 if nt % 2 == 0 else 0)
    return ((m + 3) & ~3) * sld * 8 <= NN_RES_LDS


def nn_res_max_m(nt):
    """longest reduction whose small matrix still fits the 160 KB of LDS at nt column tiles"""
    sld = nt * 16 + (16 if nt % 2 == 0 else 0)
    return NN_RES_LDS // (sld * 8) // 4 * 4


def nn_res_reachable():
    """every resident instance (TT, NT, R4, UPPER).  UPPER is only ever requested by the QR (Q <- Q R^-1: reduction length = number
    of columns), so an UPPER instance is reachable only where a SQUARE small matrix of that width fits LDS"""
    out = set()
    for nt, ttv in NN_RES_TT.items():
        for tt in {ttv, ttv - 1 if ttv > 1 else 1}:
            for r4 in range(4):
                out.add((tt, nt, r4, 0))
                for rem4 in (0, 1):
                    if any(nn_res_fits(k, nt) and r4_class(k, nt, rem4) == r4 for k in range(16 * (nt - 1) + 1, 16 * nt + 1)):
                        out.add((tt, nt, r4, 1))
    return out


# ------------------------------------------------------------------ launch_tsgemm_ss
SS_BK = 32
SS_CASES = {(1, 1), (1, 2), (1, 3), (1, 4), (1, 5), (2, 2), (2, 3), (2, 4), (2, 5), (2, 6), (3, 5), (3, 6), (4, 5), (4, 6), (4, 7),
            (5, 6), (5, 7), (6, 7), (7, 7), (7, 8), (8, 8), (9, 9), (10, 9), (11, 9),
            (3, 3), (4, 4), (5, 4), (6, 5), (7, 5)}
SS_DEAD_REMOVED = {(4, 3), (5, 3), (7, 4), (8, 4), (11, 5), (13, 5)}     # listed until this sweep, reachable from no shape


def ss_applicable(m, k, same):
    rt, ct = (m + 15) // 16, (k + 15) // 16
    if rt < 1 or ct < 1 or rt > 10 or ct > 10:
        return False
    return (rt * 16 if same else (rt + ct) * 16) <= 288


def ssb_has_instance(rt, ct):
    return 2 <= rt <= ct and ct in (5, 6, 9) and rt + ct <= 18


def ss_pf(tpw, nq):
    return 2 if (tpw <= 4 and nq <= 6) else 1


def ss_select(rt, ct, same, blocked_knob):
    """('ssb', RT, CTL, swap) or ('ss', TPW, NQ)"""
    swap = (not same) and rt > ct
    a, b = (ct, rt) if swap else (rt, ct)
    if (not same) and blocked_knob and ssb_has_instance(a, b):
        return ("ssb", a, b, int(swap))
    ctot = rt * 16 if same else (rt + ct) * 16
    tpw = ((rt * (rt + 1) // 2 if same else rt * ct) + 7) // 8
    return ("ss", tpw, (ctot + 31) // 32)


def ss_plan(m, k, N, kn, num_cus, same=False, scale=1.0, beta=0.0, rs=None, cs=1, nsplit_req=0, ptrs_aligned=True):
    rs = k if rs is None else rs
    assert ss_applicable(m, k, same)
    rt, ct = (m + 15) // 16, (k + 15) // 16
    Npad = round_up(N, SS_BK)
    sel = ss_select(rt, ct, same, kn["ss_blocked"])
    blocked = sel[0] == "ssb"
    ctot = rt * 16 if same else (rt + ct) * 16
    tpw = ((rt * (rt + 1) // 2 if same else rt * ct) + 7) // 8
    nq = (ctot + 31) // 32
    stage_bytes = nq * 32 * SS_BK * 8
    shmem = stage_bytes if (ss_pf(tpw, nq) == 2 and not blocked) else 2 * stage_bytes + nq * 32 * 8
    cus = num_cus if num_cus > 0 else 256
    per_cu = (160 * 1024) // shmem
    reg_cap = kn["ss_percu"] if (tpw <= 4 and not blocked) else 1
    per_cu = max(min(per_cu, reg_cap), 1)
    stages = Npad // SS_BK
    nsplit = nsplit_req if nsplit_req > 0 else cus * per_cu
    nsplit = max(min(nsplit, stages // 2), 1)
    chunk = round_up((Npad + nsplit - 1) // nsplit, SS_BK)
    nsplit = (Npad + chunk - 1) // chunk
    mpad, kpad = rt * 16, ct * 16
    if blocked:
        _, a, b, swap = sel
        pipe = kn["ss_blocked"] != 2 and a * b <= 56
        launch = record(SSB, a, b, (a + b + 1) // 2, pipe, swap, 0, nsplit)
        red = reduce_plan(nsplit, mpad * kpad, mpad if swap else kpad, bool(swap), m, k, rs, cs, ptrs_aligned)
        return [launch, red]
    if (tpw, nq) not in SS_CASES:
        raise LookupError("tsgemm_ss: no instance for tiles/wave=%d chunks/thread=%d" % (tpw, nq))
    return [record(SS, tpw, nq, ss_pf(tpw, nq), 0, same, nsplit), reduce_plan(nsplit, mpad * kpad, kpad, False, m, k, rs, cs, ptrs_aligned)]


def ss_tile_shapes():
    """every (rt, ct, same) the applicability rule lets through"""
    out = [(rt, ct, False) for rt in range(1, 11) for ct in range(1, 11) if (rt + ct) * 16 <= 288]
    return out + [(rt, rt, True) for rt in range(1, 11)]


def ss_reachable():
    """(set of (TPW, NQ) of the round-robin kernel, set of (RT, CTL, PIPE) of the blocked kernel) over every tile shape and
    every setting of ss_blocked"""
    ss, ssb = set(), set()
    for rt, ct, same in ss_tile_shapes():
        for knob in (0, 1, 2):
            sel = ss_select(rt, ct, same, knob)
            if sel[0] == "ss":
                ss.add(sel[1:])
            else:
                ssb.add((sel[1], sel[2], int(knob != 2 and sel[1] * sel[2] <= 56)))
    return ss, ssb


# ------------------------------------------------------------------ case lists of the GPU sweep
TN_REMS = (1, 4, 5, 8, 9, 12, 13, 16)
R4_REMS = {1: (1, 4), 2: (5, 8), 3: (9, 12), 0: (13, 16)}      # both boundaries of every R4 class
TN_SINGLE_N = (33, 64, 95)
SCALE_BETA = ((1.0, 0.0), (0.5, 0.0), (-2.0, 1.0), (1.0, -2.0), (0.5, 0.5))


def _tn_rows(mode, mt, nt, idx):
    """m and the tn_mt knob for which tn_tile gives MT = mt: the binding limit (table, need, knob) and the raggedness of the last
    row block (m % 16 in {1, 15, 0}) rotate with idx"""
    waves = 8 if mode == 8 else 4
    table = TN_MT_MAX[4 if mode == 4 else 8][nt]
    ragged = (15, 1, 0)[idx % 3]                 # rows missing from the last 16-row tile
    if mt == table:
        return (waves * mt + 1) * 16 - ragged, 0                              # the table binds: two row blocks
    if mt == 6 and table == 8 and idx % 2 == 0:
        return (waves * 6 + 1) * 16 - ragged, 0                               # need = 7, for which there is no instance: 6
    if idx % 2 == 0:
        return (waves * (mt - 1) + 1 + idx % waves) * 16 - ragged, 0          # the need binds: one ragged row block
    return (waves * table + 3) * 16 - ragged, mt                              # the knob binds: several row blocks


def tn_cases(nt_filter=None, mode_filter=None):
    """the tn sweep: dicts with the knobs, the shape and the call arguments.  Every entry of tn_reachable() appears, every R4 class
    at both boundaries of its remainder range, rem4 = 0 once per (mode 8, NT), both output orders, scale / beta rotated.  The
    rotations run on different periods (row raggedness idx % 3, N (idx // 3) % 3, remainder boundary by tr + mt + nt) so that
    their combinations occur"""
    cases = []
    idx = 0
    for nt in range(1, 17):
        for mode in ((4,) if nt > 11 else (8, 4, 44)):
            if (nt_filter is not None and nt != nt_filter) or (mode_filter is not None and mode != mode_filter):
                continue
            table = TN_MT_MAX[4 if mode == 4 else 8][nt]
            for mt in range(1, table + 1):
                if mt == 7:
                    continue
                for tr in (0, 1):
                    for r4 in ((0, 1, 2, 3) if mode == 8 else (0,)):
                        idx += 1
                        rem = R4_REMS[r4][(tr + mt + nt) % 2] if mode == 8 else TN_REMS[idx % 8]
                        m, tn_mt = _tn_rows(mode, mt, nt, idx)
                        sb = SCALE_BETA[idx % len(SCALE_BETA)]
                        cases.append({"knobs": {"ss": 0, "waves": mode, "tn_mt": tn_mt}, "m": m, "k": 16 * (nt - 1) + rem,
                                      "N": TN_SINGLE_N[(idx // 3) % 3], "tr": tr, "scale": sb[0], "beta": sb[1], "nsplit": 0,
                                      "want": (mode, mt, nt, tr, r4)})
            if mode == 8:
                # rem4 = 0: a short last tile as a full tile
                idx += 1
                m, tn_mt = _tn_rows(mode, table, nt, idx)
                cases.append({"knobs": {"ss": 0, "waves": 8, "rem4": 0, "tn_mt": tn_mt}, "m": m, "k": 16 * (nt - 1) + (1, 8, 12)[nt % 3],
                              "N": TN_SINGLE_N[(idx // 3) % 3], "tr": nt % 2, "scale": 1.0, "beta": 0.0, "nsplit": 0,
                              "want": (8, table, nt, nt % 2, 0)})
    return cases


def tn_split_cases():
    """forced splits (the partial-sum kernels at their boundaries), every route of launch_reduce_partials, the hybrid plan"""
    cases = []
    for i, (ns, N) in enumerate([(2, 32 * 16 * 2 + 1), (5, 32 * 16 * 5 + 1), (33, 32 * 16 * 33 + 1), (32, 32 * 32), (40, 32 * 40)]):
        for tr in (0, 1):
            sb = SCALE_BETA[(i + tr) % len(SCALE_BETA)]
            cases.append({"knobs": {"ss": 0}, "m": 129 + 15 * tr, "k": (74, 33, 9, 17, 138)[i], "N": N, "tr": tr, "scale": sb[0], "beta": sb[1],
                          "nsplit": ns, "ld": "odd"})
    # m k >= 65536: the vector kernel over one long row (row-major, ld = the partials') and row by row (even fast extent, even ld);
    # m k < 65536 <= m kpad with ld = kpad: the flat kernel; an odd fast extent or an odd ld: the scalar kernel
    cases.append({"knobs": {"ss": 0}, "m": 1024, "k": 64, "N": 1025, "tr": 0, "scale": 0.5, "beta": 0.0, "nsplit": 2, "ld": "kpad"})
    cases.append({"knobs": {"ss": 0}, "m": 1024, "k": 61, "N": 1025, "tr": 0, "scale": -2.0, "beta": 1.0, "nsplit": 2, "ld": "kpad"})
    cases.append({"knobs": {"ss": 0}, "m": 1024, "k": 64, "N": 1025, "tr": 1, "scale": 0.5, "beta": 0.5, "nsplit": 2, "ld": "even"})
    cases.append({"knobs": {"ss": 0}, "m": 1023, "k": 65, "N": 1025, "tr": 1, "scale": 1.0, "beta": -2.0, "nsplit": 2, "ld": "even"})
    cases.append({"knobs": {"ss": 0}, "m": 1024, "k": 64, "N": 1280, "tr": 0, "scale": 1.0, "beta": 0.0, "nsplit": 40, "ld": "even"})
    cases.append({"knobs": {"ss": 0}, "m": 1025, "k": 64, "N": 1280, "tr": 0, "scale": 1.0, "beta": 0.0, "nsplit": 40, "ld": "odd"})
    cases.append({"knobs": {"ss": 0}, "m": 1024, "k": 61, "N": 1280, "tr": 0, "scale": 0.5, "beta": 0.5, "nsplit": 40, "ld": "kpad"})
    # one output row of odd length >= 65536: the vector kernel must leave it to the scalar kernel, not drop its last element
    cases.append({"knobs": {"ss": 0}, "m": 65537, "k": 1, "N": 65, "tr": 1, "scale": 1.0, "beta": 0.0, "nsplit": 2, "ld": "even"})
    return cases


def exact_amplitude(n_reduce):
    """largest power of two a with n_reduce * a^2 <= 2^51, at most 2^19: integer operands in [-a, a] keep every partial sum of a
    reduction of that length below 2^51, hence exact in fp64 in any summation order"""
    e = 19
    while n_reduce * (1 << (2 * e)) > (1 << 51):
        e -= 1
    return 1 << e


def nn_stream_cases(num_cus=256):
    """streaming nn sweep (nn_res = 0): every entry of nn_stream_reachable(); N = two tiles plus a ragged rest"""
    cases = []
    idx = 0
    ms = (1, 31, 32, 33, 100)
    for nt in range(1, 17):
        tt4, tt8 = NN_CASE[nt]
        variants = [(8, 0, tt8)] + [(4, sel, tt) for sel, tt in ((1, tt4), (2, max(tt4 - 1, 1)), (3, max(tt4 - 2, 1)))]
        seen = set()
        for waves, nn_tt, tt in variants:
            if (waves, tt) in seen:
                continue
            seen.add((waves, tt))
            for r4 in range(4):
                idx += 1
                rem = R4_REMS[r4][idx % 2]
                rest = (32, 1, 31)[idx % 3]
                ab = ((1.0, 0.0), (0.5, 0.0), (1.0, 1.0), (-2.0, 0.5))[idx % 4]
                cases.append({"knobs": {"nn_res": 0, "nn_waves": waves, "nn_tt": nn_tt}, "N": 2 * 16 * tt * waves + rest, "m": ms[idx % 5],
                              "r": 16 * (nt - 1) + rem, "alpha": ab[0], "beta": ab[1], "inplace": False, "want": (tt, nt, waves, r4)})
        idx += 1
        cases.append({"knobs": {"nn_res": 0, "nn_waves": 8, "rem4": 0}, "N": 2 * 128 * tt8 + 31, "m": 33, "r": 16 * (nt - 1) + (4, 9)[nt % 2],
                      "alpha": 1.0, "beta": 0.0, "inplace": False, "want": (tt8, nt, 8, 0)})
    return cases


def nn_res_cases():
    """resident nn sweep: every non-UPPER entry of nn_res_reachable().  Per width the reduction length rotates over the longest
    the 160 KB of LDS hold (nn_res_max_m: 1280 rows at one column tile), three rows below it (the same padded height) and a short
    ragged one; the ragged N, beta and the remainder boundary rotate on other periods, so the longest reduction meets every N"""
    cases = []
    for nt, ttv in NN_RES_TT.items():
        j = 0
        for sel, tt in ((1, ttv), (2, ttv - 1 if ttv > 1 else 1)):
            if sel == 2 and tt == ttv:
                continue
            for r4 in range(4):
                m = (nn_res_max_m(nt), nn_res_max_m(nt) - 3, 37)[j % 3]
                cases.append({"knobs": {"nn_res_tt": sel}, "N": 4096 + (0, 1, 127)[(j + j // 3) % 3], "m": m,
                              "r": 16 * (nt - 1) + R4_REMS[r4][(j // 4 + r4) % 2], "alpha": (1.0, 0.5)[j % 2], "beta": (0.0, -2.0)[(j // 2) % 2],
                              "inplace": False, "want": (tt, nt, r4, 0)})
                j += 1
    return cases


def nn_upper_cases():
    """Q <- Q R^-1 through orthogonalize(): every UPPER entry of nn_res_reachable()"""
    cases = []
    seen = set()
    for rem4 in (1, 0):
        for nt, ttv in NN_RES_TT.items():
            for sel, tt in ((1, ttv), (2, ttv - 1 if ttv > 1 else 1)):
                for k in range(16 * (nt - 1) + 1, 16 * nt + 1):
                    r4 = r4_class(k, nt, rem4)
                    if not nn_res_fits(k, nt) or (tt, nt, r4) in seen:
                        continue
                    seen.add((tt, nt, r4))
                    cases.append({"knobs": {"nn_res_tt": sel, "rem4": rem4}, "N": 4096 + (0, 1, 127)[len(cases) % 3], "k": k,
                                  "want": (tt, nt, r4, 1)})
    return cases


def ss_cases():
    """skinny sweep: every tile shape under every setting of ss_blocked, the one-operand Gram for rt = 1..10.  Raggedness, N and the
    forced split rotate with the shape and are shifted by the knob, so every kernel family meets each of them"""
    cases = []
    for s, (rt, ct, same) in enumerate(ss_tile_shapes()):
        for knob in ((1,) if same else (0, 1, 2)):
            q = s + knob
            m = rt * 16 - (0, 1, 15)[q % 3]
            k = m if same else ct * 16 - (15, 0, 1)[(q // 3) % 3]
            sb = SCALE_BETA[q % len(SCALE_BETA)]
            cases.append({"knobs": {"ss_blocked": knob}, "m": m, "k": k, "N": (65, 2049)[(s + knob // 2) % 2], "same": same,
                          "tr": (q // 2) % 2, "scale": sb[0], "beta": sb[1], "nsplit": (0, 0, 3)[(s // 2 + knob) % 3], "rt": rt, "ct": ct})
    return cases


def out_ld(case, fast):
    """leading dimension of the test's output array: wider than the fast extent by a guard band"""
    kind = case.get("ld")
    if kind == "kpad":
        assert not case["tr"]
        return round_up(case["k"], 16)
    if kind == "even":
        return (fast + 3) // 2 * 2
    if kind == "odd":
        return (fast + 2) // 2 * 2 + 1
    ld = fast + 3
    return ld + 1 if (not case["tr"] and ld == round_up(case["k"], 16)) else ld


# more row blocks than CUs: whole rounds coarsely split + a finely split tail, with a scale that rules out the direct write
TN_HYBRID_CASE = {"knobs": {"ss": 0, "tn_mt": 1}, "m": 261 * 128 - 15, "k": 9, "N": 1025, "tr": 0, "scale": 0.5, "beta": 0.0, "nsplit": 0}
# a long reduction against a single row tile: nn_plan splits the reduction axis
NN_MSPLIT_CASE = {"knobs": {"nn_res": 0, "nn_waves": 8}, "N": 200, "m": 2048, "r": 100, "alpha": 1.0, "beta": 0.0, "inplace": False}


def nn_tail_split_case(num_cus):
    """one round of whole tiles of the shortest tile (NT = 16: 128 rows) plus three tail tiles that are split over the reduction axis"""
    return {"N": (num_cus + 3) * 128, "m": 512, "r": 250, "alpha": 1.0, "beta": 0.0, "inplace": False}
