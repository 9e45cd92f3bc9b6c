"""CPU suite: every prototype of include/hfmi.h that takes a mutable ``hfmi_block`` has a contract case in
tests/test_gpu_block_contract.py (``WRITERS``) or an explicit, reasoned exemption (``NOT_A_WRITER``).  An entry point added to the
header without either fails here, before anything runs on a GPU."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _contract_module():
    spec = importlib.util.spec_from_file_location("_block_contract_table", os.path.join(ROOT, "tests", "test_gpu_block_contract.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _header_statements():
    with open(os.path.join(ROOT, "include", "hfmi.h")) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)            # comments
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)             # preprocessor lines
    return [" ".join(s.split()) for s in text.split(";")]


def mutable_block_prototypes():
    """names of the functions (and function-pointer typedefs) with a parameter ``hfmi_block*`` / ``hfmi_block**`` that is not const"""
    names = []
    for stmt in _header_statements():
        m = re.search(r"\(\s*\*\s*(\w+)\s*\)\s*\((.*)\)\s*$", stmt) or re.search(r"(\w+)\s*\((.*)\)\s*$", stmt)
        if not m:
            continue
        params = m.group(2).split(",")
        if any(re.search(r"\bhfmi_block\s*\*", p) and not re.search(r"\bconst\s+hfmi_block\b", p) for p in params):
            names.append(m.group(1))
    return names


def all_prototypes():
    return {m.group(1) for stmt in _header_statements()
            for m in [re.search(r"\(\s*\*\s*(\w+)\s*\)\s*\(.*\)\s*$", stmt) or re.search(r"(\w+)\s*\(.*\)\s*$", stmt)] if m}


def test_the_header_parse_finds_what_the_header_has_today():
    found = set(mutable_block_prototypes())
    expected = {"hfmi_block_create", "hfmi_block_wrap", "hfmi_block_view", "hfmi_block_destroy", "hfmi_block_upload",
                "hfmi_block_upload_async", "hfmi_block_zero", "hfmi_block_copy", "hfmi_block_scale", "hfmi_block_axpy", "hfmi_randn_fill",
                "hfmi_philox_raw", "hfmi_block_fill_matern32", "hfmi_block_gemm_small", "hfmi_amg_vcycle", "hfmi_post_apply_fn",
                "hfmi_op_apply", "hfmi_allreduce", "hfmi_bcast", "hfmi_borth_qr", "hfmi_double_pass", "hfmi_double_pass_g",
                "hfmi_single_pass", "hfmi_single_pass_g", "hfmi_sketch_eig", "hfmi_bench_tsgemm_nn"}
    assert expected <= found, sorted(expected - found)
    # read-only entry points are not caught
    assert not found & {"hfmi_block_download", "hfmi_block_dot", "hfmi_block_norms", "hfmi_block_info", "hfmi_block_gram_eig",
                        "hfmi_bench_tsgemm_tn", "hfmi_op_snapshot_gram"}


def test_every_mutable_block_entry_point_has_a_contract_case_or_a_reasoned_exemption():
    mod = _contract_module()
    covered = {name for w in mod.WRITERS for name in w.covers}
    missing = [n for n in mutable_block_prototypes() if n not in covered and n not in mod.NOT_A_WRITER]
    assert not missing, "no contract case in tests/test_gpu_block_contract.py for: %s" % ", ".join(missing)


def test_the_tables_name_only_what_the_header_has():
    mod = _contract_module()
    have = all_prototypes()
    stale = sorted({name for w in mod.WRITERS for name in w.covers} - have)
    assert not stale, "WRITERS names entry points the header does not declare: %s" % stale
    mutable = set(mutable_block_prototypes())
    for name, reason in mod.NOT_A_WRITER.items():
        assert name in mutable, "%s is exempted but the header has no such prototype with a mutable block" % name
        assert isinstance(reason, str) and len(reason) > 10
    both = sorted(set(mod.NOT_A_WRITER) & {name for w in mod.WRITERS for name in w.covers})
    assert not both, "both covered and exempted: %s" % both


def test_the_table_is_well_formed_and_needs_no_gpu_to_build():
    mod = _contract_module()
    names = [w.name for w in mod.WRITERS]
    assert len(names) == len(set(names))
    for w in mod.WRITERS:
        assert callable(w.run) and w.shapes and w.modes and set(w.modes) <= set(mod.MODES)
    # the shape lists hold what they promise
    ns = {N for N, _ in mod.SHAPES}
    assert {n % 32 for n in ns} >= {0, 1, 2, 3, 31} and min(ns) < 32 and 4225 in ns and max(ns) > 65536 and max(ns) <= 2 ** 17
    assert {k for _, k in mod.SHAPES} >= {1, 5, 16, 17, 74, 138}
    # hfmi_block_dot on each side of the 65536-element switch of the partial-sum reduction.  The reduction only runs when tn_panel
    # splits the long axis: not on the skinny x skinny kernel ((ceil(m/16) + ceil(k/16)) * 16 <= 288 with both <= 160), and with at
    # least 2 x 16 stages of 32 rows.  Shapes that do not meet this never reach the switch, whatever m * k is.
    def reaches_the_reduction(N, m, k):
        rt, ct = (m + 15) // 16, (k + 15) // 16
        skinny = rt <= 10 and ct <= 10 and (rt + ct) * 16 <= 288
        return not skinny and ((N + 31) // 32) // 2 >= 16
    split = [(N, m, k) for N, m, k in mod.DOT_EXTRA if reaches_the_reduction(N, m, k)]
    assert any(m * min(k, 256) >= 65536 for _, m, k in split) and any(m * k < 65536 and k <= 256 for _, m, k in split)
    assert any(k > 256 for _, _, k in split)
