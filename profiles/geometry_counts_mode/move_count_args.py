#!/usr/bin/env python3
"""The parent's sources with ONE change: the ragged kernels' count pointers moved to the end of their parameter lists (and of
their launch calls), fps_reg_ragged_kernel given the unused npoints pointer. What differs between this tree's kernels and the
parent's is the effect of the argument order alone; what differs between this tree's and the branch's is the refactor's."""
import re, sys

csrc = sys.argv[1]
CNT = r"const int \*__restrict__ (lengths2|lengths1|lengths)"


def move_sig(s, name):
    i = s.index("void %s(" % name)
    j = s.index(")\n{", i)
    sig = s[i:j]
    found = [m.group(0) for m in re.finditer(CNT, sig)]
    assert found, name
    for f in found:
        sig = re.sub(re.escape(f) + r",\s*", "", sig, count=1)
    sig += ", " + ", ".join(found)
    return s[:i] + sig + s[j:]


def move_launch(s, name, names):
    """every launch(...) whose kernel is `name`: arguments `names` go to the end"""
    out, pos = "", 0
    for m in re.finditer(r"(auto kern = %s[<;])|(launch\(%s,)" % (name, name), s):
        i = s.index("launch(", m.start())
        j = s.index(");", i)
        call = s[i:j]
        moved = []
        for n in names:
            if re.search(r"(?<![\w.])%s," % n, call):
                call = re.sub(r"(?<![\w.])%s,\s*(\\\n\s*)?" % n, "", call, count=1)
                moved.append(n)
        call += ", " + ", ".join(moved)
        out += s[pos:i] + call
        pos = j
    return out + s[pos:]


def edit(fn, kernels, names):
    p = csrc + "/" + fn
    s = open(p).read()
    for k in kernels:
        s = move_sig(s, k)
        s = move_launch(s, k, names)
    open(p, "w").write(s)


edit("ball_query.hip", ["ball_query_ragged_kernel", "ball_query_ragged_pair_kernel", "ball_query_cells_ragged_kernel",
                        "ball_query_cells_ragged_pair_kernel"], ["lengths", "lengths2"])
edit("ball_query_msg.hip", ["ball_query_msg_ragged_kernel", "ball_query_msg_ragged_pair_kernel"], ["lengths1", "lengths2"])
edit("topk.hip", ["knn_wave_ragged_kernel", "knn_wave_ragged_pair_kernel"], ["lengths1", "lengths2"])
edit("interpolate.hip", ["three_nn_ragged_kernel", "three_nn_ragged_pair_kernel", "three_nn_cells_ragged_kernel",
                         "three_nn_cells_ragged_pair_kernel"], ["lengths", "lengths2"])
p = csrc + "/fps.hip"
s = open(p).read()
s = s.replace("""void fps_reg_ragged_kernel(int n, int m, const float *__restrict__ xyz, const int *__restrict__ lengths,
""", """void fps_reg_ragged_kernel(int n, int m, const float *__restrict__ xyz, const int *__restrict__ lengths, const int *__restrict__ npoints,
""")
s = s.replace("return launch(kern, dim3(b), dim3(T), lds, st, n, m, inp, lengths, out, oxyz);",
              "return launch(kern, dim3(b), dim3(T), lds, st, n, m, inp, lengths, npoints, out, oxyz);")
open(p, "w").write(s)
