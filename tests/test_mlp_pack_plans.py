"""The host side of the fused inference MLPs, pinned to recorded values (CPU; no device work): what pn2_sa_mlp3_config /
_ws_bytes / _pool_supported / _pack and pn2_fp_mlp_config / _ws_bytes / _pack return for every stack of
tests/mlp_exact_cases.py, against tests/golden/mlp_pack_plans.json. The packed arrays are compared through their SHA-256,
everything else value by value, all with ==. The weights come from an integer formula (no library's random stream):

    layer L (0-based), row k, column j:  float32((k 7919 + j 104729 + L 1000003 + 12345) mod 16777213) / 2^23 - 1
    bias of layer L, channel j:          the same with k = 0 and L + 7 in place of L

(the integer is below 2^24 and the division is by a power of two, so only the subtraction rounds, and IEEE fixes how).

The fixture records the library of the commit named in its "recorded_from" entry -- the one BEFORE the host code was
reorganised into plans -- and is re-recorded on purpose only:

    PN2OPS_LIBRARY=/path/to/that/libpn2ops.so python tests/test_mlp_pack_plans.py <commit>
"""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np
import pytest

import mlp_exact_cases as C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mlp_pack_plans.json")
# shapes tests/test_abi.py and test_sa_mlp_pack.py::test_config_limits expect to be refused: (cin, c1, c2, c3, nsample)
REJECTED = [(3, 64, 64, 128, 24), (3, 512, 512, 512, 32), (259, 512, 512, 1024, 32), (2, 64, 64, 128, 32), (3, 64, 64, 128, 48),
            (3, 64, 64, 128, 0)]


def _values(rows, cols, layer):
    k, j = np.arange(rows, dtype=np.int64)[:, None], np.arange(cols, dtype=np.int64)[None, :]
    v = ((k * 7919 + j * 104729 + layer * 1000003 + 12345) % 16777213).astype(np.float32)
    return np.ascontiguousarray(v / np.float32(2 ** 23) - np.float32(1), dtype=np.float32)


def _layers(cin, widths):
    dims = (cin,) + tuple(widths)
    ws = [_values(dims[i], dims[i + 1], i) for i in range(len(widths))]
    bs = [np.ascontiguousarray(_values(1, dims[i + 1], i + 7)[0]) for i in range(len(widths))]
    return ws, bs


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _lib():
    from pointnet2_amd import _C
    return _C.lib()


def sa_record(cin, widths, ns, xyz_first, group_all=False):
    lib = _lib()
    c1, c2, c3 = widths
    info, wf, bf = (ctypes.c_int * 4)(), ctypes.c_longlong(), ctypes.c_longlong()
    rec = {"config_rc": lib.pn2_sa_mlp3_config(cin, c1, c2, c3, ns, info, ctypes.byref(wf), ctypes.byref(bf)),
           "ws_bytes": lib.pn2_sa_mlp3_ws_bytes(2, 100, 7, cin, c1, c2, c3, ns),
           "pool_supported": [lib.pn2_sa_mlp3_pool_supported(cin, c1, c2, c3, ns, p) for p in range(4)]}
    if group_all:
        rec["ws_bytes_group_all"] = lib.pn2_sa_mlp3_ws_bytes(2, 100, 1, cin, c1, c2, c3, 100)
    if rec["config_rc"] != 0:
        return rec
    rec.update(info4=list(info), w_floats=wf.value, b_floats=bf.value)
    ws, bs = _layers(cin, widths)
    wp, bp = np.full(wf.value, np.nan, np.float32), np.full(bf.value, np.nan, np.float32)
    rec["pack_rc"] = lib.pn2_sa_mlp3_pack(cin, c1, c2, c3, ns, 1 if xyz_first else 0, ws[0].ctypes.data, bs[0].ctypes.data,
                                          ws[1].ctypes.data, bs[1].ctypes.data, ws[2].ctypes.data, bs[2].ctypes.data,
                                          wp.ctypes.data, bp.ctypes.data)
    rec.update(wpacked_sha256=_sha(wp), bpacked_sha256=_sha(bp))
    return rec


def fp_record(c2, c1, widths, kind):
    lib = _lib()
    n = len(widths)
    warr = (ctypes.c_int * n)(*widths)
    tiles, wf, bf = (ctypes.c_int * 4)(), ctypes.c_longlong(), ctypes.c_longlong()
    rec = {"config_rc": lib.pn2_fp_mlp_config(c2, c1, n, warr, kind, tiles, ctypes.byref(wf), ctypes.byref(bf)),
           "ws_bytes": lib.pn2_fp_mlp_ws_bytes(2, 7, c2, c1, n, warr, kind)}
    if rec["config_rc"] != 0:
        return rec
    rec.update(tiles4=list(tiles), w_floats=wf.value, b_floats=bf.value)
    ws, bs = _layers(c2 + c1, widths)
    wp, bp = np.full(wf.value, np.nan, np.float32), np.full(bf.value, np.nan, np.float32)
    wptr = (ctypes.c_void_p * n)(*[w.ctypes.data for w in ws])
    bptr = (ctypes.c_void_p * n)(*[b.ctypes.data for b in bs])
    rec["pack_rc"] = lib.pn2_fp_mlp_pack(c2, c1, n, warr, kind, wptr, bptr, wp.ctypes.data, bp.ctypes.data)
    rec.update(wpacked_sha256=_sha(wp), bpacked_sha256=_sha(bp))
    return rec


def _wname(widths):
    return "x".join(map(str, widths))


def cases():
    """{id: (recorder, args)} of everything the fixture holds."""
    table = {}
    for _, cfeat, widths, ns in C.SA_STACKS:
        table["sa-c%d-%s-ns%d" % (cfeat, _wname(widths), ns)] = (sa_record, (3 + cfeat, tuple(widths), ns, True))
    for _, cfeat, widths, ns in C.FEATURES_FIRST:
        table["sa-c%d-%s-ns%d-featfirst" % (cfeat, _wname(widths), ns)] = (sa_record, (3 + cfeat, tuple(widths), ns, False))
    for _, _, cfeat in C.GROUP_ALL:
        table["sa-group_all-c%d-%s" % (cfeat, _wname(C.GROUP_ALL_WIDTHS))] = (sa_record, (3 + cfeat, tuple(C.GROUP_ALL_WIDTHS), 100, True, True))
    for c2, c1, widths in C.FP_STACKS:
        for kind in (0, 1):
            table["fp-%d-%d-%s-kind%d" % (c2, c1, _wname(widths), kind)] = (fp_record, (c2, c1, tuple(widths), kind))
    for cin, c1, c2, c3, ns in REJECTED:
        table["rejected-cin%d-%s-ns%d" % (cin, _wname((c1, c2, c3)), ns)] = (sa_record, (cin, (c1, c2, c3), ns, True))
    return table


CASES = cases()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_fixture_lists_every_case(golden):
    assert sorted(golden["cases"]) == sorted(CASES)
    assert golden["recorded_from"]


@pytest.mark.parametrize("case", sorted(CASES))
def test_plan_and_packed_bytes_are_the_recorded_ones(golden, case):
    fn, args = CASES[case]
    assert fn(*args) == golden["cases"][case]


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit("usage: PN2OPS_LIBRARY=<library of the recorded commit> python tests/test_mlp_pack_plans.py <commit>")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = {"recorded_from": sys.argv[1], "cases": {name: fn(*args) for name, (fn, args) in sorted(CASES.items())}}
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d cases into %s" % (len(out["cases"]), GOLDEN))
