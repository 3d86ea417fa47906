"""The integer logic that csrc/cost_lines.hip::cl_tile settles once per sample instead of once per gather iteration, restated and checked
on the CPU over its whole domain:

  1. the chunk of a cell column by a multiplication (``cl_chunk_magic``): umulhi(x, ceil(2^32 / (Wc - 1))) == x // (Wc - 1);
  2. "taken from the chunk products unless behind": the rule of the descriptor pass (a band sample is gathered exactly when its chunk is not
     behind the furthest chunk an earlier band sample of the lane reached) against the cursor it replaces, which walked the samples in
     order while the chunks advanced and re-derived in / behind / consume from the packed word in every iteration;
  3. the gather's single unsigned comparison on the band-linear index against the two column comparisons it replaces.
"""
import numpy as np

CL_T, CL_RMAX = 128, 32
WCS = sorted({CL_T // R for R in range(1, CL_RMAX)})      # bands with chunks have R <= 31


def chunk_magic(Wc):
    return (0xFFFFFFFF // max(Wc - 1, 2) + 1) & 0xFFFFFFFF


def test_chunk_of_a_column_by_multiplication():
    x = np.arange(0, 1 << 15, dtype=np.uint64)             # cl_check: source maps of at most 16000 texels a side (+ the border)
    for Wc in WCS:
        assert Wc - 1 >= 3
        m = np.uint64(chunk_magic(Wc))
        assert np.array_equal((x * m) >> np.uint64(32), x // np.uint64(Wc - 1)), Wc


def cursor(kinds, chunks, nchunks):
    """The replaced gather: -> per sample 'in' (chunk products), 'behind' / 'direct' (direct path), 'zero'.  kinds: 0 band, 1 zero, 2 direct."""
    out, i = [None] * len(kinds), 0
    for n in range(nchunks):
        while i < len(kinds):
            k = kinds[i]
            if k == 0 and chunks[i] > n:
                break                                      # ahead: waits for its chunk
            out[i] = {1: "zero", 2: "direct"}.get(k) or ("in" if chunks[i] == n else "behind")
            i += 1
    for j in range(i, len(kinds)):                         # the tail behind the chunk loop
        out[j] = {0: "behind", 1: "zero", 2: "direct"}[kinds[j]]
    return out


def descriptor_pass(kinds, chunks):
    out, run = [], 0
    for k, n in zip(kinds, chunks):
        isin = k == 0 and n >= run
        run = n if isin else run
        out.append("zero" if k == 1 else "in" if isin else "behind" if k == 0 else "direct")
    return out


def test_descriptor_pass_classifies_like_the_cursor():
    rng = np.random.default_rng(7)
    seen = set()
    for _ in range(4000):
        ns, nchunks = int(rng.integers(1, 9)), int(rng.integers(1, 9))
        kinds = rng.choice([0, 0, 0, 1, 2], size=ns).tolist()
        walk = np.sort(rng.integers(0, nchunks, size=ns)) if rng.random() < 0.5 else rng.integers(0, nchunks, size=ns)
        chunks = walk.tolist()
        a, b = cursor(kinds, chunks, nchunks), descriptor_pass(kinds, chunks)
        # a band sample the cursor never reached inside the loop cannot exist: every band sample's chunk is < nchunks
        assert a == b, (kinds, chunks, nchunks, a, b)
        seen.update(b)
    assert seen == {"in", "behind", "zero", "direct"}


def test_gather_range_test_is_the_two_column_comparisons():
    for R in range(1, CL_RMAX):
        Wc = CL_T // R
        span = (Wc - 1) * R
        for cb in (-131, -2, 0, 7, 15990):
            for col in range(cb - 3, cb + Wc + 3):         # cell column; the packed word carries col + 4
                for r0 in range(0, max(R - 1, 0)):          # a band sample's row: r0 + 1 < R
                    old = cb + 4 <= col + 4 <= cb + Wc - 2 + 4
                    t0 = ((col + 4) * R + r0 - (cb + 4) * R) & 0xFFFFFFFF
                    assert (t0 < span) == old, (R, cb, col, r0)
        assert 0x40000000 - (-131 + 4) * R > span and ((0x40000000 - (16010 + 4) * R) & 0xFFFFFFFF) > span      # "no sample left"
