"""Host arithmetic behind tests/test_igemm_forms_{cpu,gpu}.py, written from the descriptor and the documented launch rules of
csrc/conv_igemm.hip - not from the library: the class table of a launch (rows, taps, K-steps and tiles per class) and an
enumerator of the stream-K unit space that names the structures a launch contains."""

STRUCTURES = "abcdefgh"


def out_hw(case):
    G, N, h, w, cin, cout, k, st, pad = case
    return (h + 2 * pad - k) // st + 1, (w + 2 * pad - k) // st + 1


def class_table(case, dgrad):
    """[(rows per group, taps, K per tap)] of the launch's classes, in launch order.  Forward and stride-1 backward-data: one
    class over every tap.  Stride-2 backward-data: one class per parity (py, px) of the dx pixel, over the taps r with
    (py + pad - r) even (likewise s); classes without taps are not part of the launch; the others run longest K first, equal
    lengths in (py, px) order."""
    G, N, h, w, cin, cout, k, st, pad = case
    ho, wo = out_hw(case)
    if not dgrad:
        return [(N * ho * wo, k * k, cin)]
    cls = []
    for py in range(st):
        for px in range(st):
            sub_h, sub_w = len(range(py, h, st)), len(range(px, w, st))
            nr = len([r for r in range(k) if (py + pad - r) % st == 0])
            ns = len([s for s in range(k) if (px + pad - s) % st == 0])
            if sub_h > 0 and sub_w > 0 and nr * ns > 0:
                cls.append((N * sub_h * sub_w, nr * ns, cout))
    return sorted(cls, key=lambda c: -c[1] * c[2])       # stable: equal K keeps the parity order


def class_counts(case, dgrad, bm, bn, bk):
    """(tiles, K-steps per tile) per class for a bm x bn tile stepping K by bk."""
    G, N, h, w, cin, cout, k, st, pad = case
    ncols = cin if dgrad else cout
    ntiles = -(-ncols // bn)
    tab = class_table(case, dgrad)
    return [G * -(-rows // bm) * ntiles for rows, _, _ in tab], [max(-(-taps * kc // bk), 1) for _, taps, kc in tab]


def streamk_structures(cls_tiles, cls_kt, P):
    """The set of structures (letters of STRUCTURES) in a stream-K launch of P workgroups over the unit space that runs class by
    class, tile by tile, K-step by K-step, workgroup b taking the units [b*U//P, (b+1)*U//P):
      a  a tile held whole by one workgroup
      b  a tile shared by exactly two workgroups
      c  a tile shared by three or more: some workgroup's whole share is a middle piece
      d  a workgroup holding the tail of one tile and the head of the next and nothing else (both slab slots used)
      e  a workgroup holding the tail of a tile, one or more whole tiles, and the head of another
      f  a cut between two workgroups that falls exactly on a tile boundary
      g  more than one class, and a cut strictly inside a tile of each class
      h  classes with different K lengths"""
    assert len(cls_tiles) == len(cls_kt) and P >= 1
    bounds, cls_of = [0], []                      # tile boundaries in units, class of each tile
    for ci, (nt, kt) in enumerate(zip(cls_tiles, cls_kt)):
        for _ in range(nt):
            bounds.append(bounds[-1] + kt)
            cls_of.append(ci)
    U = bounds[-1]
    cuts = [b * U // P for b in range(P + 1)]
    found = set()
    owners = [0] * len(cls_of)                    # workgroups with a piece of each tile
    for b in range(P):
        u0, u1 = cuts[b], cuts[b + 1]
        if u1 == u0:
            continue
        pieces = []                               # (starts the tile, ends the tile) per tile this workgroup touches
        for t in range(len(cls_of)):
            lo, hi = max(u0, bounds[t]), min(u1, bounds[t + 1])
            if lo < hi:
                owners[t] += 1
                pieces.append((lo == bounds[t], hi == bounds[t + 1]))
        whole = [p for p in pieces if p == (True, True)]
        if whole:
            found.add("a")
        if len(pieces) == 1 and pieces[0] == (False, False):
            found.add("c")
        tail_first = not pieces[0][0] and len(pieces) > 1
        head_last = not pieces[-1][1] and len(pieces) > 1
        if tail_first and head_last:
            found.add("d" if len(pieces) == 2 else "e")
    if any(n == 2 for n in owners):
        found.add("b")
    if any(n >= 3 for n in owners):
        found.add("c")
    inner = set(bounds[1:-1])
    if any(c in inner for c in cuts[1:-1]):
        found.add("f")
    if len(cls_tiles) > 1:
        cut_in = set()
        for c in cuts[1:-1]:
            for t in range(len(cls_of)):
                if bounds[t] < c < bounds[t + 1]:
                    cut_in.add(cls_of[t])
        if cut_in == set(range(len(cls_tiles))):
            found.add("g")
        if len(set(cls_kt)) > 1:
            found.add("h")
    return found


# ---- the cases of tests/test_igemm_forms_gpu.py (G, N, h, w, cin, cout, k, stride, pad), kept here so that the host-side
# checks of test_igemm_forms_cpu.py read the same lists.  `cus`: the CUs left to the planners (the rest reserved).
FWD, BWD = "fwd", "bwd"

# stream-K: (direction, case, cus, (bm, bn, bk), persistent workgroups P, structures) - P and the structures as an MI355X
# (256 CUs; 2 / 5 resident workgroups of the forward 128x128 / 128x64 kernels, 3 / 5 of the backward-data ones) plans them
STREAMK_CASES = [
    (FWD, (1, 6, 15, 15, 512, 256, 3, 1, 1), 8, (128, 128, 32), 16, "abdef"),    # 22 tiles x 144 K-steps, 198 per workgroup
    (FWD, (1, 5, 15, 15, 512, 128, 3, 1, 1), 8, (128, 128, 32), 16, "bcd"),      # 9 tiles: 81 K-steps per workgroup
    (FWD, (1, 3, 15, 15, 512, 64, 3, 1, 1), 8, (128, 64, 16), 40, "cdf"),        # 6 tiles x 288 over 40 workgroups
    (BWD, (1, 16, 15, 15, 128, 256, 3, 1, 1), 9, (128, 128, 16), 27, "abde"),    # 29 tiles x 144
    (BWD, (1, 5, 16, 16, 128, 512, 3, 1, 1), 8, (128, 128, 16), 24, "cdf"),      # 10 tiles x 288
    (BWD, (1, 3, 15, 15, 64, 512, 3, 1, 1), 8, (128, 64, 16), 40, "cdf"),
    (BWD, (1, 9, 11, 13, 128, 1024, 3, 2, 1), 16, (128, 128, 16), 48, "bcdfgh"),  # stride 2: 4 classes x 3 tiles, 256/128/128/64 K-steps
    (BWD, (1, 5, 11, 13, 64, 1024, 3, 2, 1), 12, (128, 64, 16), 60, "cdfgh"),
    (BWD, (1, 2, 17, 18, 64, 256, 7, 2, 3), 12, (128, 64, 16), 60, "cdfgh"),      # 7x7 stride 2: 16 / 12 / 12 / 9 taps
]
# one tile per workgroup at 8 CUs: (direction, case, (bm, bn, bk, uniform-tap loader))
PLAIN_CASES = [
    (FWD, (1, 1, 31, 31, 64, 256, 1, 1, 0), (128, 128, 32, True)),      # 16 tiles, ragged last row tile
    (FWD, (1, 1, 31, 31, 8, 256, 3, 1, 1), (128, 128, 32, False)),      # 8 channels per tap: the general loader
    (FWD, (1, 2, 31, 31, 32, 64, 3, 1, 1), (128, 64, 16, True)),
    (FWD, (1, 2, 31, 31, 8, 64, 3, 1, 1), (128, 64, 16, False)),
    (FWD, (1, 3, 9, 9, 64, 64, 3, 1, 1), (64, 64, 16, True)),
    (FWD, (1, 3, 9, 9, 8, 64, 3, 1, 1), (64, 64, 16, False)),
    (FWD, (1, 3, 9, 9, 16, 32, 3, 1, 1), (128, 32, 16, False)),
    (BWD, (1, 1, 31, 31, 256, 16, 3, 1, 1), (128, 128, 16, True)),
    (BWD, (1, 1, 31, 31, 256, 8, 3, 1, 1), (128, 128, 16, False)),
    (BWD, (1, 2, 31, 31, 64, 16, 3, 1, 1), (128, 64, 16, True)),
    (BWD, (1, 2, 31, 31, 64, 8, 3, 1, 1), (128, 64, 16, False)),
    (BWD, (1, 3, 9, 9, 64, 64, 3, 1, 1), (64, 64, 16, True)),
    (BWD, (1, 3, 9, 9, 64, 8, 3, 1, 1), (64, 64, 16, False)),
    (BWD, (1, 3, 9, 9, 32, 16, 3, 1, 1), (128, 32, 16, False)),
]
PLAIN_CUS = 8
# weight gradient: (case, (bm rows of cout, bn columns of r*s*cin, incremental pixel addressing))
WGRAD_CASES = [
    ((1, 3, 7, 7, 128, 128, 1, 1, 0), (128, 128, True)),
    ((1, 5, 5, 5, 128, 160, 1, 1, 0), (128, 128, False)),     # ho * wo = 25, ragged second row tile
    ((2, 2, 6, 6, 16, 64, 3, 1, 1), (64, 128, True)),         # 144 columns: ragged second column tile
    ((1, 7, 1, 1, 128, 64, 1, 1, 0), (64, 128, False)),       # 7 pixels in a 16-pixel K-step
    ((1, 2, 8, 8, 96, 64, 1, 1, 0), (64, 64, True)),
    ((1, 4, 2, 2, 64, 96, 1, 1, 0), (64, 64, False)),
    ((1, 2, 13, 13, 64, 32, 3, 2, 1), (32, 128, True)),       # stride 2, ho * wo = 49
    ((1, 3, 5, 5, 32, 32, 3, 1, 1), (32, 128, False)),
    ((1, 2, 6, 6, 32, 64, 1, 1, 0), (128, 32, True)),         # cout >= 64, r*s*cin < 64
    ((1, 3, 4, 4, 32, 64, 1, 1, 0), (128, 32, False)),
    ((1, 2, 7, 7, 4, 64, 3, 1, 1), (128, 32, True)),          # 36 columns: two column tiles, the second ragged
]
WGRAD_SPLITS_CASE = (1, 16, 8, 8, 256, 256, 3, 1, 1)          # 36 tiles, 1024 pixels: 4 splits on every CU, one on 8
