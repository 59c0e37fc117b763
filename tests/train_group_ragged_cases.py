"""The cases of the masked grouped training node (train_mlp.sa_mlp_train(..., counts=), pn2_mlp_train_*_group_ragged), shared by
tests/test_train_group_ragged_gpu.py (which runs them) and tests/test_train_group_ragged_plan.py (which proves on the CPU that
their union reaches every masked kernel instantiation the node adds). The smallest shapes where each piece can go wrong:

  a   b 4, n 256, m 32, nsample 16, cfeat 8, 11 -> 32 -> 32 -> 64, lengths (256, 200, 40, 130), counts (32, 17, 1, 24): odd counts
      with nsample 16 leave a validity word half valid; a cloud of one group.
  b   (a) without features (3 -> 32 -> 64), nsample 32, m 16, b 3: coordinates only (no data gradient at layer 1).
  c   (a) with xyz_first=False: the MSG channel order.
  d   group_all: b 4, n 128, cfeat 64, 67 -> 128 -> 256, counts (128, 77, 1, 32): partial words inside the one group, a cloud of
      one point.
  ea, ed   (a) and (d) with a one-layer stack: layer 1 is also the top layer.
  f*  the wide ones the plan test needs, 16,384 rows (b 4, m 128, nsample 32) with 128- and 256-wide layers: NS 2 and 4 of the
      gathered GEMM with resident and with streamed weights, and the gathered weight gradient's (TPW, UPW) pairs beyond (1, 1).
      `opts` are train_mlp.options() overrides.

idx case: `lengths` are the clouds' point counts (idx of a valid group names rows below them), `counts` their centroid counts.
group_all: `counts` are the point counts."""

A = dict(b=4, n=256, m=32, ns=16, cfeat=8, widths=[32, 32, 64], lengths=(256, 200, 40, 130), counts=(32, 17, 1, 24))
D = dict(b=4, n=128, m=1, ns=128, cfeat=64, widths=[128, 256], counts=(128, 77, 1, 32), group_all=True)
_WIDE = dict(b=4, n=512, m=128, ns=32, lengths=(512, 300, 64, 411), counts=(128, 77, 1, 50))

CASES = {
    "a": A,
    "b": dict(b=3, n=256, m=16, ns=32, cfeat=0, widths=[32, 64], lengths=(256, 200, 40), counts=(16, 9, 1)),
    "c": dict(A, xyz_first=False),
    "d": D,
    "ea": dict(A, widths=[32]),
    "ed": dict(D, widths=[128]),
    "f_ns4": dict(_WIDE, cfeat=8, widths=[256, 256]),                       # NS 4 resident; weight gradient (1, 3)
    "f_ns2_w12": dict(_WIDE, cfeat=8, widths=[128]),                        # NS 2 resident; (1, 2)
    "f_131": dict(_WIDE, cfeat=128, widths=[256]),                          # five input tiles in one slab: (2, 2)
    "f_131_ns2": dict(_WIDE, cfeat=128, widths=[256], opts=dict(max_ns=2)),
    "f_131_stream": dict(_WIDE, cfeat=128, widths=[256], opts=dict(force_stream=True)),       # NS 4 streamed
    "f_131_ns2_stream": dict(_WIDE, cfeat=128, widths=[256], opts=dict(max_ns=2, force_stream=True)),
    "f_ns1_stream": dict(A, opts=dict(force_stream=True)),                  # NS 1 streamed
    "f_64": dict(_WIDE, cfeat=61, widths=[256]),                            # two input tiles x eight output tiles: (2, 3)
    "f_256": dict(_WIDE, cfeat=253, widths=[256]),                          # four x eight: (4, 3)
}
CAPTURE = ("a", "d")                                                        # capture + replay under new counts
NEW_COUNTS = {"a": (5, 32, 20, 1), "d": (9, 128, 64, 33)}


def dims(case):
    """-> b, n, m, nsample, cfeat, has_idx, widths (cin_1, cout_1 .. cout_L)"""
    return (case["b"], case["n"], case["m"], case["ns"], case["cfeat"], not case.get("group_all", False),
            [3 + case["cfeat"]] + list(case["widths"]))
