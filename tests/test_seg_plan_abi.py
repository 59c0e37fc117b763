"""CPU tests of the index-plan part of the C ABI (include/pn2ops.h "index plans", csrc/seg_grad.hip): the size and layout queries
are host logic, the header declares what the library exports, the two structs that gained a trailing `idx_plan` have the
compiler's size in their ctypes mirrors, and argument errors come back before anything is launched (no GPU here)."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["pn2_seg_plan_bytes", "pn2_seg_plan_layout", "pn2_group_point_plan", "pn2_three_interpolate_plan",
       "pn2_group_point_grad_planned", "pn2_three_interpolate_grad_planned", "pn2_group_point_grad_planned_ex",
       "pn2_three_interpolate_grad_planned_ex", "pn2_fp_interp_concat_grad_planned"]

SHAPES = [(4, 500, 70 * 16), (4, 1024, 625 * 32), (4, 600, 625 * 64), (3, 500, 70 * 16), (4, 25000, 94 * 32), (4, 2, 192), (1, 1, 0),
          (32, 512, 128 * 64)]


def _lib():
    from pointnet2_amd import _C
    return _C.lib()


def _layout(b, rows, entries):
    off = (ctypes.c_longlong * 5)()
    lf, cap = ctypes.c_int(0), ctypes.c_longlong(0)
    assert _lib().pn2_seg_plan_layout(b, rows, entries, off, ctypes.byref(lf), ctypes.byref(cap)) == 0
    return list(off), lf.value, cap.value


def test_new_symbols_are_bound_and_exported():
    from pointnet2_amd import _C
    lib = ctypes.CDLL(_C.LIB_PATH)
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in _C.EXPORTED, n
    import pointnet2_amd
    assert callable(pointnet2_amd.index_plan)


@pytest.mark.parametrize("b,rows,entries", SHAPES)
def test_plan_bytes_hold_the_workspace_and_the_table(b, rows, entries):
    lib = _lib()
    cap = entries // 32 + 1
    assert lib.pn2_seg_plan_bytes(b, rows, entries) >= lib.pn2_seg_grad_ws_bytes(b, rows, entries) + 4 * (b + b * cap)


def test_plan_bytes_are_monotone_in_each_argument():
    lib = _lib()
    for b, rows, entries in SHAPES:
        base = lib.pn2_seg_plan_bytes(b, rows, entries)
        assert lib.pn2_seg_plan_bytes(b + 1, rows, entries) >= base
        assert lib.pn2_seg_plan_bytes(b, rows + 1, entries) >= base
        assert lib.pn2_seg_plan_bytes(b, rows, entries + 1) >= base
        assert lib.pn2_seg_plan_bytes(b, rows, entries + 32) > base
    assert lib.pn2_seg_plan_bytes(0, 10, 10) == 16 and lib.pn2_seg_plan_bytes(2, 0, 10) == 16 and lib.pn2_seg_plan_bytes(2, 10, -1) == 16


@pytest.mark.parametrize("b,rows,entries", SHAPES)
def test_plan_layout(b, rows, entries):
    lib = _lib()
    off, long_from, cap = _layout(b, rows, entries)
    sizes = [4 * b * (rows + 1), 4 * b * rows, 4 * b * entries, 4 * b, 4 * b * cap]       # start, sorted, list, long_count, long_rows
    assert off[0] == 0
    for k in range(5):
        assert off[k] % 4 == 0
        if k:
            assert off[k] >= off[k - 1] + sizes[k - 1]                                     # ordered, no overlap
    assert off[4] + sizes[4] <= lib.pn2_seg_plan_bytes(b, rows, entries)
    assert off[1] >= sizes[0] + 4 * b * rows                                               # the build's cursor scratch sits between
    assert cap == entries // 32 + 1
    want = ctypes.c_int(0)
    assert lib.pn2_seg_grad_plan(rows, entries, 64, b * rows, ctypes.byref(want), None) == 0
    assert long_from == want.value and long_from >= 32
    assert cap * long_from > entries                                                       # the table cannot overflow


def test_plan_layout_argument_errors():
    lib = _lib()
    assert lib.pn2_seg_plan_layout(0, 10, 10, None, None, None) == -2
    assert lib.pn2_seg_plan_layout(1, 0, 10, None, None, None) == -2
    assert lib.pn2_seg_plan_layout(1, 10, -1, None, None, None) == -2
    assert lib.pn2_seg_plan_layout(1, 10, 10, None, None, None) == 0


def test_argument_errors_come_before_any_launch():
    """No GPU on this machine: a call that reached a launch would return a hipError_t (> 0)."""
    lib = _lib()
    one = ctypes.c_void_p(16)                                      # a non-NULL pointer nothing may read through
    # shapes
    assert lib.pn2_group_point_plan(-1, 8, 2, 2, one, 0, one, None) == -2
    assert lib.pn2_group_point_plan(1, 0, 2, 2, one, 0, one, None) == -2
    assert lib.pn2_group_point_plan(1, 8, -2, 2, one, 0, one, None) == -2
    assert lib.pn2_three_interpolate_plan(1, 8, 0, one, 0, one, None) == -2
    assert lib.pn2_three_interpolate_plan(1, -8, 4, one, 0, one, None) == -2
    assert lib.pn2_group_point_grad_planned(1, 0, 4, 2, 2, one, one, one, 0, None) == -2
    assert lib.pn2_group_point_grad_planned(1, 8, 0, 2, 2, one, one, one, 0, None) == -2
    assert lib.pn2_group_point_grad_planned(1, 8, -4, 2, 2, one, one, one, 0, None) == -2
    assert lib.pn2_group_point_grad_planned(-1, 8, 4, 2, 2, one, one, one, 0, None) == -2
    assert lib.pn2_three_interpolate_grad_planned(1, 8, 4, 0, one, one, one, one, 0, None) == -2
    assert lib.pn2_three_interpolate_grad_planned(1, 8, 0, 4, one, one, one, one, 0, None) == -2
    assert lib.pn2_three_interpolate_grad_planned(1, -1, 4, 4, one, one, one, one, 0, None) == -2
    # NULL pointers
    assert lib.pn2_group_point_plan(1, 8, 2, 2, one, 0, None, None) == -1
    assert lib.pn2_group_point_plan(1, 8, 2, 2, None, 0, one, None) == -1
    assert lib.pn2_three_interpolate_plan(1, 8, 4, one, 1, None, None) == -1
    assert lib.pn2_three_interpolate_plan(1, 8, 4, None, 1, one, None) == -1
    assert lib.pn2_group_point_grad_planned(1, 8, 4, 2, 2, one, None, one, 0, None) == -1
    assert lib.pn2_group_point_grad_planned(1, 8, 4, 2, 2, None, one, one, 0, None) == -1
    assert lib.pn2_group_point_grad_planned(1, 8, 4, 2, 2, one, one, None, 0, None) == -1
    assert lib.pn2_three_interpolate_grad_planned(1, 8, 4, 4, one, None, one, one, 1, None) == -1
    assert lib.pn2_three_interpolate_grad_planned(1, 8, 4, 4, one, one, None, one, 1, None) == -1
    assert lib.pn2_fp_interp_concat_grad_planned(1, 8, 4, 4, 0, 4, one, None, one, one, None, one, 0, None) == -1
    assert lib.pn2_fp_interp_concat_grad_planned(1, 8, 0, 4, 0, 4, one, one, one, one, None, one, 0, None) == -2
    # the variant of the _ex entries
    assert lib.pn2_group_point_grad_planned_ex(1, 8, 4, 2, 2, one, one, one, 0, 3, None) == -3
    assert lib.pn2_group_point_grad_planned_ex(1, 8, 4, 2, 2, one, one, one, 0, -1, None) == -3
    assert lib.pn2_three_interpolate_grad_planned_ex(1, 8, 4, 4, one, one, one, one, 0, 7, None) == -3
    # a plan that is not 4-byte aligned
    assert lib.pn2_group_point_grad_planned(1, 8, 4, 2, 2, one, ctypes.c_void_p(18), one, 0, None) == -3
    assert lib.pn2_group_point_plan(1, 8, 2, 2, one, 0, ctypes.c_void_p(18), None) == -3
    # nothing to do
    assert lib.pn2_group_point_plan(0, 8, 2, 2, None, 0, None, None) == 0
    assert lib.pn2_three_interpolate_plan(0, 8, 4, None, 0, None, None) == 0
    assert lib.pn2_group_point_grad_planned(0, 8, 4, 2, 2, None, None, None, 0, None) == 0
    assert lib.pn2_three_interpolate_grad_planned(0, 8, 4, 4, None, None, None, None, 0, None) == 0
    assert lib.pn2_group_point_plan(2, 8, 0, 4, None, 0, one, None) == 0          # no references: the gradient reads no plan
    assert lib.pn2_three_interpolate_plan(2, 0, 4, None, 0, one, None) == 0


def test_header_compiles_as_c_links_and_gives_the_struct_sizes(tmp_path):
    """A C program with nothing but the header links the new symbols; the two structs that gained `idx_plan` have the size and
    field offsets of the ctypes mirrors; a zero-initialised pn2_group_src / pn2_fp_src has idx_plan == NULL."""
    from pointnet2_amd import _C, train_mlp
    checks = [("pn2_group_src", train_mlp.GroupSrc), ("pn2_fp_src", train_mlp.FpSrc)]
    body = ['#include "pn2ops.h"', "#include <stdio.h>", "#include <stddef.h>", "#include <string.h>", "int main(void) {",
            "long long off[5]; int lf = 0; long long cap = 0;",
            "pn2_group_src g; pn2_fp_src f;", "memset(&g, 0, sizeof g); memset(&f, 0, sizeof f);"]
    for cname, py in checks:
        body.append('printf("%s %%zu", sizeof(%s));' % (cname, cname))
        for fname, _ in py._fields_:
            body.append('printf(" %%zu", offsetof(%s, %s));' % (cname, fname))
        body.append('printf("\\n");')
    body += ['printf("null %d %d\\n", g.idx_plan == NULL, f.idx_plan == NULL);',
             'printf("bytes %lld %d\\n", pn2_seg_plan_bytes(4, 500, 1120), pn2_seg_plan_layout(4, 500, 1120, off, &lf, &cap));',
             'printf("rc %d %d %d %d %d %d %d\\n", pn2_group_point_plan(1, 8, 2, 2, 0, 0, 0, 0), pn2_three_interpolate_plan(1, 8, 4, 0, 0, 0, 0),',
             '       pn2_group_point_grad_planned(1, 8, 4, 2, 2, 0, 0, 0, 0, 0), pn2_three_interpolate_grad_planned(1, 8, 4, 4, 0, 0, 0, 0, 0, 0),',
             '       pn2_group_point_grad_planned_ex(1, 8, 4, 2, 2, 0, 0, 0, 0, 9, 0), pn2_three_interpolate_grad_planned_ex(1, 8, 4, 4, 0, 0, 0, 0, 0, 9, 0),',
             '       pn2_fp_interp_concat_grad_planned(1, 8, 4, 4, 0, 4, 0, 0, 0, 0, 0, 0, 0, 0));',
             "return 0; }"]
    src = tmp_path / "plan.c"
    src.write_text("\n".join(body) + "\n")
    exe = tmp_path / "plan"
    libdir = os.path.dirname(_C.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-L", libdir, "-lpn2ops", "-Wl,-rpath," + libdir, "-o", str(exe)], check=True, capture_output=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    for line, (cname, py) in zip(lines, checks):
        parts = line.split()
        assert parts[0] == cname
        assert int(parts[1]) == ctypes.sizeof(py), cname
        assert [int(v) for v in parts[2:]] == [getattr(py, f).offset for f, _ in py._fields_], cname
        assert py._fields_[-1][0] == "idx_plan"
    assert ctypes.sizeof(train_mlp.GroupSrc) == 64 and ctypes.sizeof(train_mlp.FpSrc) == 64      # the sizes the header states
    assert lines[2] == "null 1 1"
    assert lines[3] == "bytes %d 0" % _lib().pn2_seg_plan_bytes(4, 500, 1120)
    assert lines[4] == "rc -1 -1 -1 -1 -3 -3 -1"


def test_index_plan_host_checks():
    """IndexPlan.check and index_plan's argument checks are host logic."""
    import torch
    import pointnet2_amd as P
    from pointnet2_amd.index_plan import IndexPlan
    plan = IndexPlan(torch.zeros(8, dtype=torch.int32), 2, 10, 12, "group", False)
    plan.check("group", 2, 10, 12, torch.device("cpu"))
    for args in (("interpolate", 2, 10, 12), ("group", 3, 10, 12), ("group", 2, 11, 12), ("group", 2, 10, 24)):
        with pytest.raises(ValueError):
            plan.check(*args, torch.device("cpu"))
    with pytest.raises(ValueError):
        P.index_plan(torch.zeros(2, 3, 4, dtype=torch.int32), 10, "gather")
    with pytest.raises(ValueError):
        P.index_plan(torch.zeros(2, 3, 4, dtype=torch.int32), 10, "group")          # not on a device: there is no CPU path
