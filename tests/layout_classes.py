"""The layout classes of the track-description chain (ofdis_bof.hip, ofdis_kmeans.hip), derived from the launchers' own choices
through the host-only hooks of the test library (tests/launch_hooks.py: bof_shape, km_geom, km_finish_split).  No GPU.

Everything behind the descriptors sees a layout (nxy, nt) through C = nxy^2 nt alone: channels of 8 C (HOG, MBHx, MBHy) and
9 C (HOF) entries in rows of 33 C bytes.  What a kernel does differently from one C to the next is stated here once, as the
class of C; tests/test_descriptor_layout_classes.py holds the layout lists of the GPU tests to a member of every class, and the
table of DESIGN.md (section 4, track description) is table() below:

    python tests/layout_classes.py      # prints it"""
import collections

from launch_hooks import bof_shape, km_finish_split, km_geom

PAIRS = [(nxy, nt) for nxy in range(1, 5) for nt in range(1, 9)]   # the public ranges: 32 pairs, 28 values of C

Class = collections.namedtuple("Class", "variant nk cut_fragment cut_kstep el np passes cut_pass mod4 finish")


def cells(size):
    return size[0] * size[0] * size[1]


def layout_class(C):
    """variant: (NK, TG) of the assignment kernel; nk: the k-steps of the 8 C and the 9 C channel; cut_fragment, cut_kstep: a
    channel ends inside a 16-byte fragment, inside a k-step of 64 bytes; el, np: the lanes and passes of the k-means sum;
    passes: the passes that hold dwords of the 8 C and the 9 C channel; cut_pass: the last of them ends inside the pass; mod4:
    9 C mod 4, the bytes of the 9 C channel's last dword (0: whole); finish: the finish kernel's entries at a time on either"""
    lens = (8 * C, 9 * C)
    _, NK, TG = bof_shape(C)
    np_, el, _ = km_geom(C)
    nd = [(n + 3) // 4 for n in lens]
    return Class(variant=(NK, TG), nk=tuple(-(-n // 64) for n in lens), cut_fragment=any(n % 16 for n in lens),
                 cut_kstep=any(n % 64 for n in lens), el=el, np=np_, passes=tuple(-(-d // el) for d in nd),
                 cut_pass=tuple(d % el != 0 for d in nd), mod4=9 * C % 4, finish=tuple(km_finish_split(n) for n in lens))


def sum_class(C):
    """the part of the class the k-means sum sees"""
    c = layout_class(C)
    return c.el, c.np, c.passes, c.cut_pass, c.mod4


def finish_class(C):
    return layout_class(C).finish


def missing(layouts, key=layout_class):
    """the classes (by `key`) that occur over PAIRS and have no member in `layouts`, each with the values of C that have it"""
    have = {key(cells(s)) for s in layouts}
    lost = collections.defaultdict(set)
    for s in PAIRS:
        if key(cells(s)) not in have:
            lost[key(cells(s))].add(cells(s))
    return {k: sorted(v) for k, v in lost.items()}


def table():
    """the markdown table of DESIGN.md: one row per C, and which tests run it beyond the sweep over every layout"""
    import test_gpu_bof as B
    import test_gpu_kmeans as K
    smallest = min(B.DESC_CASES, key=lambda c: c[0] * c[1])
    marks = (("W", B.SECOND_WORKGROUP_LAYOUTS), ("S", B.LAYOUTS + B.STRUCTURED_LAYOUTS), ("L", K.LAYOUTS + K.LONG_SEGMENT_LAYOUTS),
             ("T", K.LAYOUTS + K.TAIL_BYTES_LAYOUTS), ("E", [B.END_TO_END_16_CELLS[7:], smallest[7:]]))
    marks = [(m, {cells(s) for s in which}) for m, which in marks]   # (a class is a matter of C alone)
    rows = ["| C | nxy, nt | assignment `<NK, TG>` | k-steps 8 C / 9 C | sum `(el, np)` | passes 8 C / 9 C | 9 C mod 4 | finish split | tests |",
            "|---|---|---|---|---|---|---|---|---|"]
    for s in B.SWEEP_LAYOUTS:
        C = cells(s)
        c = layout_class(C)
        cut = lambda v, is_cut: f"{v} cut" if is_cut else f"{v}"
        tests = ("full" if s in B.LAYOUTS else "sweep") + "".join(" " + m for m, which in marks if C in which)
        rows.append(f"| {C} | {s[0]}, {s[1]} | `<{c.variant[0]}, {c.variant[1]}>` | {c.nk[0]} / {c.nk[1]} | `({c.el}, {c.np})` | "
                    f"{cut(c.passes[0], c.cut_pass[0])} / {cut(c.passes[1], c.cut_pass[1])} | {c.mod4} | {c.finish[0]} / {c.finish[1]} | "
                    f"{tests} |")
    return "\n".join(rows)


if __name__ == "__main__":
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "tools")]
    print(table())
