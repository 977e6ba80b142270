"""CPU checks of the ensemble entries (include/ocn_sw.h ocn_ens_*): the ctypes mirrors of the new
structs against the header (gcc probe, as tests/test_abi.py), the planner's invariants over a grid of
inputs (ocn_ens_plan is pure: no device), and a loud failure of ocn_ens_create without a device."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "ocn_sw.h")

STRUCTS = {"ocn_ens_group": "OcnEnsGroup", "ocn_ens_info_t": "OcnEnsInfo"}


@pytest.fixture(scope="module")
def lib():
    import ocean_model_arch_amd as amd
    if not os.path.exists(amd._lib.LIB_PATH):
        amd.build()
    return amd.lib()


def test_struct_layouts_and_abi_version(lib, tmp_path):
    from ocean_model_arch_amd import _lib
    assert lib.ocn_abi_version() == 5
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {"]
    for cs, py in STRUCTS.items():
        lines.append(f'printf("{cs} size %zu\\n", sizeof({cs}));')
        for fname, _ in getattr(_lib, py)._fields_:
            lines.append(f'printf("{cs} {fname} %zu\\n", offsetof({cs}, {fname}));')
    lines.append('printf("max %d cap %d\\n", OCN_ENS_MAX_MEMBERS, OCN_ENS_OPT_CAPACITY);')
    lines.append("return 0; }")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    for line in out:
        w = line.split()
        if not w:
            continue
        if w[0] == "max":
            assert (int(w[1]), int(w[3])) == (_lib.ENS_MAX_MEMBERS, _lib.ENS_OPT_CAPACITY)
            continue
        py = getattr(_lib, STRUCTS[w[0]])
        if w[1] == "size":
            assert C.sizeof(py) == int(w[2]), line
        else:
            assert getattr(py, w[1]).offset == int(w[2]), line


def _block(W, H):
    from ocean_model_arch_amd import _lib
    return _lib.OcnBlock(3, W + 2, 3, H + 2, 1, W + 4, 1, H + 4, W + 4)


def _tiles(W, H, rows):
    return -(-W // 60) * -(-H // (4 * rows))


def test_tile_formula_examples(lib):
    from ocean_model_arch_amd.ensemble import plan
    assert (_tiles(61, 9, 1), _tiles(121, 65, 1), _tiles(241, 151, 1)) == (6, 51, 190)
    for (W, H), t in (((61, 9), 6), ((121, 65), 51), ((241, 151), 190)):
        g, = plan(_block(W, H), [0], 512)
        assert (g["rows"], g["tiles"], g["members"], g["first_tile"]) == (1, t, [0], [0])


MEMBERS = (1, 2, 3, 9, 34)
BLOCKS = ((1, 1), (61, 9), (121, 65), (241, 151), (1525, 1115))
CAPS = (7, 60, 256, 512)
# variant patterns over the member index: one variant; three mixed; mixed with ineligible members
PATTERNS = {"one": lambda i: 4, "mixed": lambda i: (0, 7, 3)[i % 3], "holes": lambda i: (-1, 2, 11, -3, 2)[i % 5]}


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
def test_planner_invariants(lib, pattern):
    from ocean_model_arch_amd.ensemble import plan
    for M, (W, H), cap in itertools.product(MEMBERS, BLOCKS, CAPS):
        what = f"{pattern} M={M} {W}x{H} cap={cap}"
        var = [PATTERNS[pattern](i) for i in range(M)]
        groups = plan(_block(W, H), var, cap)
        eligible = [i for i in range(M) if var[i] >= 0]
        if _tiles(W, H, 16) > cap:   # a block that does not fit alone at 16 rows: nobody is eligible
            assert groups == [], what
            continue
        seen = [i for g in groups for i in g["members"]]
        assert sorted(seen) == eligible, what                      # every eligible member in exactly one group
        for g in groups:
            n = len(g["members"])
            assert n >= 1 and {var[i] for i in g["members"]} == {g["variant"]}, what   # one variant per group
            assert g["members"] == sorted(g["members"]), what
            assert g["tiles"] == _tiles(W, H, g["rows"]) and 1 <= g["rows"] <= 16, what
            assert g["first_tile"] == [j * g["tiles"] for j in range(n)], what          # the running sums
            assert n * g["tiles"] <= cap, what                                           # resident at once
        for v in set(var[i] for i in eligible):
            mine = [g for g in groups if g["variant"] == v]
            nv = sum(var[i] == v for i in eligible)
            fits = [r for r in range(1, 17) if nv * _tiles(W, H, r) <= cap]
            rows = {g["rows"] for g in mine}
            if fits:   # the smallest rows at which the variant's members fit together: one group
                assert len(mine) == 1 and rows == {fits[0]}, what
            else:      # 16 rows, floor(capacity / tiles) members per launch
                per = cap // _tiles(W, H, 16)
                assert rows == {16} and [len(g["members"]) for g in mine] == \
                    [min(per, nv - k) for k in range(0, nv, per)], what


def test_planner_rejects_bad_input(lib):
    from ocean_model_arch_amd import _lib
    b = _block(61, 9)
    v = (C.c_int32 * 2)(0, 0)
    n = C.c_int32(-1)
    assert lib.ocn_ens_plan(C.byref(b), v, 2, 0, None, 0, C.byref(n)) == _lib.OCN_ERR_ARG
    assert lib.ocn_ens_plan(C.byref(b), v, 0, 8, None, 0, C.byref(n)) == _lib.OCN_ERR_ARG
    assert lib.ocn_ens_plan(C.byref(b), None, 2, 8, None, 0, C.byref(n)) == _lib.OCN_ERR_ARG
    assert lib.ocn_ens_plan(C.byref(b), v, _lib.ENS_MAX_MEMBERS + 1, 8, None, 0, C.byref(n)) == _lib.OCN_ERR_ARG
    # a count without an output array (two variants: two groups)
    v = (C.c_int32 * 2)(0, 1)
    assert lib.ocn_ens_plan(C.byref(b), v, 2, 8, None, 0, C.byref(n)) == _lib.OCN_OK and n.value == 2


def test_loud_failure_without_device(lib):
    import ocean_model_arch_amd as amd
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if has_gpu:
        e = amd.OceanEnsemble(amd.box_config(8), members=2)
        assert len(e) == 2
        e.close()
        return
    with pytest.raises(amd.OcnError) as ei:
        amd.OceanEnsemble(amd.box_config(8), members=2)
    assert ei.value.code in (amd._lib.OCN_ERR_HIP, amd._lib.OCN_ERR_ARG)
    # argument errors come before any device call
    with pytest.raises(amd.OcnError) as ei:
        amd.OceanEnsemble(amd.box_config(8), members=0)
    assert ei.value.code == amd._lib.OCN_ERR_ARG
