"""The case table of the SIMT layer's conformance tests, with each primitive's contract stated in numpy and plain Python integers.

tests/device_prims/kw_conformance.hpp holds one kernel body per group of primitives (it calls the product's functions of kai_simt.hpp, kai_wave.hpp, kai_batch_kernels.hpp,
kai_stale_gangs.hpp, kai_fill_buckets.hpp, kai_fill_levels.hpp).  The same bodies are built twice, for the emulator (tests/test_kw_conformance.py) and for gfx950
(tests/test_gpu_kw_conformance.py); both files run the cases below and hold the result against the references below.  No reference here is taken from either build.

A case is a list of launches: (body id, grid, block, input words, preset output words, check).  `check(out)` asserts.  Inputs are seeded.  Words are uint64: doubles travel as
their bits, ints sign-extended.  Outputs are preset with FILL so that a word the body never wrote is seen.

Workgroup shapes: 64 (one wavefront, four DPP rows), 128 (two wavefronts), 256, 1 024 (sixteen wavefronts: what PlanScanLds is dimensioned for); 100 (a last wavefront of 36
lanes) and 1 for what the product calls in partial workgroups (ballot, shfl, wave_scan_add<int>, sg_wg_scan).  Patterns of every scan and reduction: all zero, all equal,
one-hot at every lane 0 .. 63 (workgroup k has its one non-zero in lane k, so a wrong DPP control or row mask shows in the lane it breaks), one-hot at every lane of the last
wavefront of a block of several, seeded random."""
import math

import numpy as np

U64 = np.uint64
M32 = (1 << 32) - 1
M64 = (1 << 64) - 1
FILL = 0xA5A5A5A5A5A5A5A5
KB_INF = 0x7FFFFFFF
IDS = dict(scan_int=0, scan_f64=1, wave_max=2, key_scan=3, block_add3=4, block_add6=5, block_max=6, block_excl=7, wg_scan=8, plan_setup=9, lane_ops=10, shfl=11,
           ballot_rank=12, scalar_bits=13, lds_ops=14, atomics=15, div_small=16, kfl_table=17)
BLOCKS = (64, 128, 256, 1024)
MAX_GRID = 64


class Launch:
    def __init__(self, body, grid, block, inp, out_words, check, preset=None):
        self.body, self.grid, self.block = IDS[body], int(grid), int(block)
        self.inp = np.ascontiguousarray(inp, dtype=U64).reshape(-1)
        self.out0 = np.full(int(out_words), FILL, U64) if preset is None else np.ascontiguousarray(preset, dtype=U64).reshape(-1)
        self.check = check


def run_case(case, kwc_run):
    """kwc_run(body, inp, out, grid, block) -> status; out is written in place"""
    n = 0
    for l in case():
        out = l.out0.copy()
        rc = kwc_run(l.body, l.inp, out, l.grid, l.block)
        assert rc == 0, f"kwc_run returned {rc} (grid {l.grid}, block {l.block})"
        l.check(out)
        n += 1
    assert n >= 1
    return n


def load_kwc_run(so):
    """the C entry point of either build (kw_conformance.hip / kw_conformance_sim.cpp) as kwc_run(body, inp, out, grid, block)"""
    import ctypes as C
    lib = C.CDLL(so)
    lib.kwc_run.restype = C.c_int
    lib.kwc_run.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int]
    return lambda body, inp, out, grid, block: lib.kwc_run(body, inp.ctypes.data, inp.nbytes, out.ctypes.data, out.nbytes, grid, block)


def _rng(*key):
    return np.random.default_rng([20260 + k for k in key])


def _i2w(a):
    """signed integers -> words (sign-extended)"""
    return np.asarray(a, dtype=np.int64).astype(U64)


def _w2i(w):
    return np.asarray(w, dtype=U64).astype(np.int64)


def _f2w(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(U64)


def _waves(block):
    return -(-block // 64)


def _chunks(rows):
    """rows: [G, ...], a workgroup each; launches of at most MAX_GRID workgroups -> (g0, g1)"""
    return [(g, min(g + MAX_GRID, len(rows))) for g in range(0, len(rows), MAX_GRID)]


def scan_patterns(block, rng, rand, one=1, equal=3):
    """[G, block] values (int64 or float64, as `rand(shape)` returns): zero, all equal, random x 4, one-hot at every lane of the first wavefront, ... of the last one"""
    nw = _waves(block)
    r = rand((4, block))
    rows = [np.zeros((1, block), r.dtype), np.full((1, block), equal, r.dtype), r]
    for w in sorted({0, nw - 1}):
        lanes = min(64, block - 64 * w)
        h = np.zeros((lanes, block), r.dtype)
        h[np.arange(lanes), 64 * w + np.arange(lanes)] = one
        rows.append(h)
    return np.concatenate(rows)


def wave_cumsum(v, block):
    """inclusive sums inside each wavefront of each workgroup, added lane by lane from lane 0 (for the exact inputs used here every order gives these bits)"""
    g, nw = v.shape[0], _waves(block)
    p = np.zeros((g, nw * 64), v.dtype)
    p[:, :block] = v
    return np.cumsum(p.reshape(g, nw, 64), axis=2).reshape(g, -1)[:, :block]


def same_f64(got_words, want, what):
    """bit-equal, but for a zero: the contract leaves a zero sum's sign open (kai_simt.hpp, wave_scan_add)"""
    want_w = _f2w(want).reshape(-1)
    got_words = np.asarray(got_words, U64).reshape(-1)
    zero = (want_w << U64(1)) == 0
    ok = (got_words == want_w) | (zero & ((got_words << U64(1)) == 0))
    assert ok.all(), f"{what}: first difference at flat index {int(np.argmin(ok))}: got {hex(int(got_words[np.argmin(ok)]))}, want {hex(int(want_w[np.argmin(ok)]))}"


def same_words(got, want, what):
    got = np.asarray(got, U64).reshape(-1)
    want = np.asarray(want, U64).reshape(-1)
    ok = got == want
    assert ok.all(), f"{what}: first difference at flat index {int(np.argmin(ok))} of {ok.size}: got {hex(int(got[np.argmin(ok)]))}, want {hex(int(want[np.argmin(ok)]))} ({int((~ok).sum())} differ)"


# ------------------------------------------------------------------------------------------------ wave_scan_add
def _scan_int(block):
    def case():
        v = scan_patterns(block, _rng(0, block), lambda s: _rng(1, block).integers(-(1 << 20), (1 << 20) + 1, s), one=-777, equal=(1 << 20))
        want = wave_cumsum(v, block)
        for g0, g1 in _chunks(v):
            yield Launch("scan_int", g1 - g0, block, _i2w(v[g0:g1]), (g1 - g0) * block, lambda out, w=want[g0:g1]: same_words(out, _i2w(w), f"wave_scan_add<int> block {block}"))
    return case


def exact_f64_sets(block, salt):
    """inputs for which every order of addition is exact: integer-valued up to 2^40, multiples of 2^-10 up to 2^20 (negative ones too), -0.0 everywhere, one subnormal among zeros"""
    r = _rng(2, block, salt)
    a = scan_patterns(block, r, lambda s: r.integers(0, 1 << 40, s).astype(np.float64), one=float((1 << 40) - 1), equal=float(1 << 39))
    b = scan_patterns(block, r, lambda s: r.integers(-(1 << 30), 1 << 30, s).astype(np.float64) / 1024.0, one=-(2.0 ** -10), equal=1.0 / 1024.0)
    c = np.full((2, block), -0.0)
    c[1, block // 2:] = 0.0
    d = np.zeros((min(block, 64), block))
    d[np.arange(len(d)), (np.arange(len(d)) * 37 + 5) % block] = 5e-324  # the smallest subnormal: only the low dword's lowest bit is set
    e = np.zeros((1, block))
    e[0, block // 3] = 2.0 ** -1030
    return np.concatenate([a, b, c, d, e])


def _scan_f64_exact(block):
    def case():
        v = exact_f64_sets(block, 0)
        want = wave_cumsum(v, block)
        for g0, g1 in _chunks(v):
            yield Launch("scan_f64", g1 - g0, block, _f2w(v[g0:g1]), (g1 - g0) * block, lambda out, w=want[g0:g1]: same_f64(out, w, f"wave_scan_add<double> (exact sums) block {block}"))
    return case


# any order of adding n non-negative doubles is within (n - 1) u / (1 - (n - 1) u) relative of the exact sum, u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, 4.2)
ROUNDING_BOUND = 63 * 2.0 ** -53 / (1 - 63 * 2.0 ** -53)


def _scan_f64_rounding(block):
    def case():
        r = _rng(3, block)
        v = np.concatenate([r.random((8, block)), r.random((4, block)) * 10.0 ** r.integers(-12, 12, (4, block)), np.exp(r.normal(0, 8, (4, block)))])
        nw = _waves(block)
        exact = np.zeros(v.shape)
        for g in range(v.shape[0]):
            for w in range(nw):
                row = v[g, 64 * w:min(64 * w + 64, block)].tolist()
                exact[g, 64 * w:64 * w + len(row)] = [math.fsum(row[:i + 1]) for i in range(len(row))]

        def check(out):
            got = out.view(np.float64).reshape(v.shape)
            err = np.abs(got - exact) / exact  # (fsum rounds the exact sum once more: half an ulp, far inside the bound's slack at short prefixes only where the bound is 0 -> lane 0 below)
            lane0 = np.zeros(v.shape, bool)
            lane0[:, ::64] = True
            assert (got[lane0] == v[lane0]).all(), "lane 0 returns its own value"
            worst = float(err[~lane0].max()) if (~lane0).any() else 0.0
            lanes = (np.arange(block) % 64)[None, :].repeat(v.shape[0], 0)
            bound = lanes * 2.0 ** -53 / (1 - lanes * 2.0 ** -53) + 2.0 ** -53  # lane l sums l + 1 terms; + the reference's own rounding
            print(f"wave_scan_add<double> rounding sums, block {block}: worst relative error {worst:.3e}, bound at lane 63 {ROUNDING_BOUND:.3e}")
            assert (err <= np.minimum(bound, ROUNDING_BOUND + 2.0 ** -53)).all(), f"a prefix is further from the exact sum than any order of addition can be: {worst:.3e}"
        yield Launch("scan_f64", v.shape[0], block, _f2w(v), v.size, check)
    return case


# ------------------------------------------------------------------------------------------------ wave_max_u64 / wave_argmax_first
def _wave_max(block):
    def case():
        r = _rng(4, block)
        nw = _waves(block)
        rows = []
        base = r.integers(1, 1 << 62, (64, block), dtype=np.uint64)  # the maximum at every lane: workgroup k, lane (k + wave) % 64 of every wavefront
        for k in range(64):
            for w in range(nw):
                base[k, 64 * w + (k + w) % 64] = (1 << 62) + k
        rows.append(base)
        rows.append(r.integers(1, 4, (8, block), dtype=np.uint64))  # ties
        tie = np.full((4, block), 9, np.uint64)  # every lane ties; ties from lane 63 down to one lane
        tie[1, :] = 1; tie[1, 63::64] = 9
        tie[2, :] = 1; tie[2, 17::64] = 9; tie[2, 48::64] = 9
        tie[3, :] = 0
        rows.append(tie)
        hi = (r.integers(0, 1 << 32, (4, block), dtype=np.uint64) << U64(32)) | U64(0x12345678)
        lo = (U64(0x00000007) << U64(32)) | r.integers(0, 1 << 32, (4, block), dtype=np.uint64)
        sw = r.integers(0, 1 << 32, (4, block), dtype=np.uint64)  # the larger key has the smaller low dword: a compare of the halves in the wrong order shows
        sw = ((sw & U64(0xff)) << U64(32)) | (U64(M32) - sw)
        top = r.integers(0, 1 << 64, (8, block), dtype=np.uint64)
        top[:4] |= U64(1 << 63) * (r.integers(0, 2, (4, block), dtype=np.uint64))
        rows += [hi, lo, sw, top]
        keys = np.concatenate(rows)
        n = r.permutation(keys.size).reshape(keys.shape).astype(np.int64) - 1000
        g_all = keys.shape[0]
        kw_ = keys.reshape(g_all, nw, 64)
        m = kw_.max(axis=2)
        first = (kw_ == m[:, :, None]).argmax(axis=2)  # the lowest lane that holds the maximum
        nwin = np.take_along_axis(n.reshape(g_all, nw, 64), first[:, :, None], axis=2)[:, :, 0]
        want = np.zeros((g_all, nw, 64, 5), U64)
        want[..., 0] = m[:, :, None]; want[..., 1] = m[:, :, None]; want[..., 3] = m[:, :, None]
        want[..., 2] = _i2w(nwin)[:, :, None]; want[..., 4] = _i2w(nwin)[:, :, None]
        want = want.reshape(g_all, block, 5)
        inp = np.stack([keys, _i2w(n)], axis=2)
        for g0, g1 in _chunks(keys):
            yield Launch("wave_max", g1 - g0, block, inp[g0:g1], (g1 - g0) * block * 5,
                         lambda out, w=want[g0:g1], g0=g0: same_words(out, w, f"wave_max_u64 / wave_argmax_first block {block} workgroups {g0}.. (per thread: max, kw key, kw n, kai key, kai n)"))
    return case


# ------------------------------------------------------------------------------------------------ PlanKey scans
def key_rows(r, shape, word):
    """PlanKeys [*shape, 4] that differ in word `word` only (word 4: in all)"""
    k = np.empty(shape + (4,), U64)
    k[...] = r.integers(1, 1 << 63, 4, dtype=np.uint64)
    if word == 4:
        k[...] = r.integers(1, 1 << 63, shape + (4,), dtype=np.uint64)
        k[..., 0] = r.integers(1, 4, shape, dtype=np.uint64)  # (a few values of w0, so that the later words decide too)
    else:
        k[..., word] = r.integers(1, 1 << 64 - 1, shape, dtype=np.uint64)
    return k


def valid_rows(r, kind, block):
    v = np.zeros(block, bool)
    if kind == "all": v[:] = True
    elif kind == "alt": v[::2] = True
    elif kind == "alt1": v[1::2] = True
    elif kind == "rand": v[:] = r.random(block) < 0.3
    elif kind == "sparse": v[:] = r.random(block) < 0.02
    elif kind == "no_wave1": v[:] = True; v[64:128] = False          # a whole wavefront without a valid key
    elif kind == "last_wave": v[64 * (_waves(block) - 1):] = True    # only the last wavefront has any
    elif kind == "none": pass
    else: v[int(kind)] = True
    return v


SMALL, LARGE = (0, 0, 0, 0), (M64, M64, M64, M64)


def running_max(keys, valid, carry):
    """inclusive running lexicographic maximum over tuples, seeded with carry (None: no carry) -> per element the maximum (None before the first key), exclusive form, last"""
    cur, inc, exc = carry, [], []
    for k, v in zip(keys, valid):
        exc.append(cur)
        if v and (cur is None or k > cur): cur = k
        inc.append(cur)
    return inc, exc, cur


def _tuples(a):
    return [tuple(x) for x in a.reshape(-1, 4).tolist()]


def _key_scan(block):
    def case():
        r = _rng(5, block)
        nw = _waves(block)
        cfgs = [(w, v, c) for w in range(5) for v in ("none", "alt", "alt1", "all", "rand", "sparse") for c in (None, SMALL, LARGE)]
        cfgs += [(k % 5, str(k), (None, SMALL)[k & 1]) for k in range(64)]  # only lane k of the first wavefront is valid (lane 64 * w + k of the others: below)
        G = len(cfgs)
        inp = np.zeros((G, block, 10), U64); want = []; cmp = []
        for g, (word, vk, carry) in enumerate(cfgs):
            keys = key_rows(r, (block,), word)
            valid = valid_rows(r, vk, block)
            if vk.isdigit():
                valid[:] = False; valid[int(vk) % 64::64] = True
            inp[g, :, :4] = keys; inp[g, :, 4] = valid; inp[g, :, 5] = carry is not None; inp[g, :, 6:] = carry or (5, 6, 7, 8)
            kt = _tuples(keys)
            for w in range(nw):
                inc, _, _ = running_max(kt[64 * w:64 * w + 64], valid[64 * w:64 * w + 64].tolist(), carry)
                want += [i or (0, 0, 0, 0) for i in inc]; cmp += [i is not None for i in inc]
        want = np.array(want, dtype=U64).reshape(G, block, 4); cmp = np.array(cmp).reshape(G, block)
        for g0, g1 in _chunks(inp):
            def check(out, g0=g0, g1=g1):
                got = out.reshape(g1 - g0, block, 4).copy()
                got[~cmp[g0:g1]] = 0  # lanes before the first valid one, without a carry: not part of the contract
                same_words(got, want[g0:g1], f"kb_wave_scan_max block {block} workgroups {g0}..")
            yield Launch("key_scan", g1 - g0, block, inp[g0:g1], (g1 - g0) * block * 4, check)
    return case


def _block_keys(body, block):
    excl = body == "block_excl"

    def case():
        r = _rng(6 + excl, block)
        kinds = ["none", "alt", "all", "rand", "sparse", "last_wave", "0", str(block - 1), str(block // 2 + 1)] + (["no_wave1"] if block >= 128 else [])
        cfgs = [(w % 5, va, vb, c) for w, (va, vb) in enumerate([(a, b) for a in kinds for b in ("rand", "none", "all")]) for c in (None, SMALL, LARGE)]
        G = len(cfgs)
        ow = 20 if excl else 16
        inp = np.zeros((G, block, 16), U64); want = np.zeros((G, block, ow), U64); cmp = np.zeros((G, block, ow), bool)
        for g, (word, va, vb, carry) in enumerate(cfgs):
            a, b = key_rows(r, (block,), word), key_rows(r, (block,), word)
            if carry is not None and g % 7 == 3: carry = tuple(a[block // 2].tolist())  # a carry in the middle of the values
            xa, xb = valid_rows(r, va, block), valid_rows(r, vb, block)
            i1, e1, l1 = running_max(_tuples(a), xa.tolist(), carry)
            i2, e2, l2 = running_max(_tuples(b), xb.tolist(), l1)
            inp[g, :, 0:4] = a; inp[g, :, 4] = xa; inp[g, :, 5:9] = b; inp[g, :, 9] = xb; inp[g, :, 10] = carry is not None; inp[g, :, 11:15] = carry or (5, 6, 7, 8); inp[g, :, 15] = l1 is not None
            z = (0, 0, 0, 0)
            if excl:  # pre[4] have_pre last[4] have_last, twice
                for o, (e, l) in ((0, (e1, l1)), (10, (e2, l2))):
                    want[g, :, o:o + 4] = [x or z for x in e]; cmp[g, :, o:o + 4] = np.array([x is not None for x in e])[:, None]
                    want[g, :, o + 4] = [x is not None for x in e]; cmp[g, :, o + 4] = True
                    want[g, :, o + 5:o + 9] = l or z; cmp[g, :, o + 5:o + 9] = l is not None
                    want[g, :, o + 9] = l is not None; cmp[g, :, o + 9] = True
            else:     # key[4] last[4], twice
                for o, (i, l) in ((0, (i1, l1)), (8, (i2, l2))):
                    want[g, :, o:o + 4] = [x or z for x in i]; cmp[g, :, o:o + 4] = np.array([x is not None for x in i])[:, None]
                    want[g, :, o + 4:o + 8] = l or z; cmp[g, :, o + 4:o + 8] = l is not None
        for g0, g1 in _chunks(inp):
            def check(out, g0=g0, g1=g1):
                got = out.reshape(g1 - g0, block, ow).copy()
                assert not (got == U64(FILL)).all(axis=2).any(), "a thread wrote nothing"
                got[~cmp[g0:g1]] = 0  # a key that does not exist (no valid element and no carry so far) is not part of the contract
                same_words(got, want[g0:g1], f"kb_{body} block {block} workgroups {g0}.. ({ow} words per thread)")
            yield Launch(body, g1 - g0, block, inp[g0:g1], (g1 - g0) * block * ow, check)
    return case


def _block_add(nv, block):
    def case():
        sets = [exact_f64_sets(block, 10 + k) for k in range(nv)]
        G = min(len(s) for s in sets)
        d = np.stack([np.roll(s[:G], 3 * k, axis=0) for k, s in enumerate(sets)], axis=2)  # [G, block, nv]: the nv sums of one workgroup see different patterns
        i1 = np.cumsum(d, axis=1); t1 = i1[:, -1:, :]
        d2 = d + d; d2[:, 0, :] = d[:, 0, :] + t1[:, 0, :]  # the second call: twice the values, thread 0 carries the first call's totals
        i2 = np.cumsum(d2, axis=1); t2 = i2[:, -1:, :]
        want = np.concatenate([i1, np.broadcast_to(t1, d.shape), i2, np.broadcast_to(t2, d.shape)], axis=2)
        for g0, g1 in _chunks(d):
            yield Launch(f"block_add{nv}", g1 - g0, block, _f2w(d[g0:g1]), (g1 - g0) * block * 4 * nv,
                         lambda out, w=want[g0:g1], g0=g0: same_f64(out, w, f"kb_block_scan_add<{nv}> block {block} workgroups {g0}.. (per thread: incl, total, incl, total of the second call)"))
    return case


# ------------------------------------------------------------------------------------------------ sg_wg_scan, kb_plan_setup
def _wg_scan(block):
    def case():
        r = _rng(8, block)
        v1 = scan_patterns(block, r, lambda s: r.integers(-(1 << 20), 1 << 20, s), one=1 | 1 << 16, equal=1 | 1 << 16)
        packed = r.choice(np.array([0, 1, 1 | 1 << 16]), (4, block))  # the two counters of kai_stale_gangs.hpp in one word
        v1 = np.concatenate([v1, packed])
        v2 = np.roll(v1, 5, axis=0)[:, ::-1].copy()
        inp = np.stack([_i2w(v1), _i2w(v2)], axis=2)
        c1, c2 = np.cumsum(v1, axis=1), np.cumsum(v2, axis=1)
        want = np.stack([c1, np.broadcast_to(c1[:, -1:], c1.shape), c2, np.broadcast_to(c2[:, -1:], c2.shape)], axis=2)
        for g0, g1 in _chunks(inp):
            yield Launch("wg_scan", g1 - g0, block, inp[g0:g1], (g1 - g0) * block * 4,
                         lambda out, w=want[g0:g1], g0=g0: same_words(out, _i2w(w), f"sg_wg_scan block {block} workgroups {g0}.. (per thread: incl, total, incl, total of the second call)"))
    return case


def _plan_setup(block):
    def case():
        for M in (1, 1023, 1024, 1025, 2185):
            r = _rng(9, block, M)
            Q, h_leaf = M - 1, 8
            nchild = np.where(r.random(M) < 0.2, r.integers(1, 6, M), 0)
            child_off = np.concatenate([[0], np.cumsum(nchild)])
            cur, rem = r.integers(0, 50, M), r.integers(-2, 21, M)
            end = cur + rem
            h_nodes = r.permutation(M)
            inp32 = np.concatenate([[Q, h_leaf], child_off, cur, end, h_nodes, [0]]).astype(np.int32)  # (one pad: an even number of 32-bit words)
            assert inp32.size == 4 * M + 4
            leaf = (np.arange(M) < Q) & (nchild == 0)
            cnt = np.where(leaf, np.clip(np.minimum(rem, h_leaf), 0, None), 0)
            ve, vk = (cnt + nchild)[h_nodes], (cnt + 1)[h_nodes]
            ebase, kbase = np.zeros(M, np.int64), np.zeros(M, np.int64)
            ebase[h_nodes] = np.cumsum(ve) - ve; kbase[h_nodes] = np.cumsum(vk) - vk
            want32 = np.concatenate([ebase, kbase, cnt, np.full(M, KB_INF), np.zeros(3 * M, np.int64), [ve.sum(), vk.sum()]]).astype(np.int32)
            out_bytes = (7 * M + 2) * 4 + M
            words = -(-out_bytes // 8)

            def check(out, M=M, want32=want32, out_bytes=out_bytes):
                raw = out.view(np.uint8)
                got32 = raw[:(7 * M + 2) * 4].view(np.int32)
                names = ["q_ebase", "q_kbase", "q_cnt", "q_sent", "q_valid", "q_nk", "q_taken"]
                for i, nm in enumerate(names):
                    assert np.array_equal(got32[i * M:(i + 1) * M], want32[i * M:(i + 1) * M]), f"kb_plan_setup block {block}, {M} nodes: {nm} differs, first at {int(np.argmax(got32[i * M:(i + 1) * M] != want32[i * M:(i + 1) * M]))}"
                assert got32[7 * M:].tolist() == want32[7 * M:].tolist(), f"plan_tot {got32[7 * M:].tolist()} != {want32[7 * M:].tolist()}"
                assert (raw[(7 * M + 2) * 4:out_bytes] == 1).all(), "q_complete"
                assert (raw[out_bytes:] == 0xA5).all(), "bytes behind the last array were written"
            yield Launch("plan_setup", 1, block, inp32.view(U64), words, check)
    return case


# ------------------------------------------------------------------------------------------------ lanes
SPECIAL_F64 = (0x8000000000000000, 0x7FF00000DEADBEEF, 0x7FF8000012345678, 0xFFF0000000000001, 0x0000000000000001, 0x00000001FFFFFFFF)  # -0.0, NaNs with payloads, a subnormal


def _lane_ops(block):
    def case():
        r = _rng(10, block)
        nw = _waves(block)
        G = 64
        v = r.integers(0, 1 << 64, (G, nw, 64), dtype=np.uint64)
        src = (np.arange(G)[:, None] + 7 * np.arange(nw)[None, :]) % 64  # workgroup k, wavefront w: from / into lane (k + 7 w) % 64
        for g in range(G):
            for w in range(nw):
                v[g, w, (src[g, w] + (g % 3) - 1) % 64] = SPECIAL_F64[(g + w) % len(SPECIAL_F64)]  # on the source lane in a third of the workgroups, next to it in the others
        u = r.integers(0, 1 << 64, (G, nw), dtype=np.uint64)
        inp = np.stack([v, np.broadcast_to(u[:, :, None], v.shape), np.broadcast_to(src[:, :, None].astype(U64), v.shape)], axis=3)
        vs = np.take_along_axis(v, src[:, :, None], axis=2)  # [G, nw, 1]: the source lane's value
        ub = np.broadcast_to(u[:, :, None], v.shape)
        at = np.arange(64)[None, None, :] == src[:, :, None]
        sx = lambda a: _i2w((a & U64(M32)).astype(np.uint32).view(np.int32).astype(np.int64))  # the low dword as an int, as a word
        want = np.stack([np.broadcast_to(sx(vs), v.shape), np.broadcast_to(vs >> U64(32), v.shape), np.broadcast_to(vs, v.shape), np.broadcast_to(vs, v.shape),
                         sx(ub), ub >> U64(32), ub, np.where(at, sx(ub), sx(v)), np.where(at, ub, v), ub, ub & U64(M32)], axis=3)
        yield Launch("lane_ops", G, block, inp, G * block * 11, lambda out: same_words(out, want, f"bcast / uni / writelane / opaque block {block} (11 words per thread: bcast int, u32, u64, f64; uni int, u32, u64; writelane int, u64; opaque u64, u32)"))
    return case


def _shfl(block):
    def case():
        r = _rng(11, block)
        nw = _waves(block)
        G = 6
        v = r.integers(0, 1 << 64, (G, block), dtype=np.uint64)
        v[0, :min(block, len(SPECIAL_F64))] = SPECIAL_F64[:min(block, len(SPECIAL_F64))]
        lane = np.arange(block) % 64
        live = np.minimum(64, block - (np.arange(block) // 64) * 64)  # lanes of the thread's wavefront that exist: only those are sources (the contract, kai_simt.hpp)
        src = np.stack([lane, live - 1 - lane, (lane + 1) % live, (lane + live - 1) % live, r.integers(0, 64, block) % live, r.integers(0, 64, block) % live])
        inp = np.stack([v, src.astype(U64)], axis=2)
        base = (np.arange(block) // 64) * 64
        got_from = np.take_along_axis(v, (base[None, :] + src), axis=1)
        sx = lambda a: _i2w((a & U64(M32)).astype(np.uint32).view(np.int32).astype(np.int64))
        cols = [sx(got_from), got_from, got_from, got_from]
        ups = []
        for d in (1, 2, 4, 8, 16, 32, 63):
            idx = np.where(lane >= d, np.arange(block) - d, np.arange(block))  # lanes below d keep their own value
            ups.append(v[:, idx])
        want = np.stack(cols + [sx(x) for x in ups] + ups, axis=2)
        yield Launch("shfl", G, block, inp, G * block * 18, lambda out: same_words(out, want, f"shfl / shfl_up block {block} (18 words per thread: shfl int, f64, u64, i64; shfl_up int by 1 2 4 8 16 32 63; shfl_up u64 likewise)"))
    return case


def _ballot_rank(block):
    def case():
        r = _rng(12, block)
        nw = _waves(block)
        G = 4 + 64
        p = np.zeros((G, nw * 64), np.uint64); m = np.zeros((G, nw), np.uint64)
        p[1] = 1; m[1] = M64
        p[2:4] = r.integers(0, 2, (2, nw * 64)) * r.integers(1, 1 << 63, (2, nw * 64))  # (any non-zero word is true)
        m[2:4] = r.integers(0, 1 << 64, (2, nw), dtype=np.uint64)
        for k in range(64):
            p[4 + k, k::64] = 1 << (k % 40)
            m[4 + k] = U64(1) << U64(k)
        exists = np.arange(nw * 64) < block  # at block 100 the lanes the last wavefront does not have count as 0
        bits = ((p != 0) & exists[None, :]).reshape(G, nw, 64)
        ball = (bits.astype(U64) << np.arange(64, dtype=U64)[None, None, :]).sum(axis=2, dtype=U64)
        below = [(1 << l) - 1 for l in range(64)]
        rank = np.array([[[bin(int(m[g, w]) & below[l]).count("1") for l in range(64)] for w in range(nw)] for g in range(G)], dtype=U64)
        inp = np.stack([p.reshape(G, nw, 64), np.broadcast_to(m[:, :, None], (G, nw, 64))], axis=3).reshape(G, nw * 64, 2)[:, :block]
        want = np.stack([np.broadcast_to(ball[:, :, None], (G, nw, 64)), rank], axis=3).reshape(G, nw * 64, 2)[:, :block]
        for g0, g1 in _chunks(inp):
            yield Launch("ballot_rank", g1 - g0, block, inp[g0:g1], (g1 - g0) * block * 2, lambda out, w=want[g0:g1], g0=g0: same_words(out, w, f"ballot / rank_below block {block} workgroups {g0}.."))
    return case


def _scalar_bits():
    def case():
        r = _rng(13)
        vals = [0, 1, 2, 1 << 31, M32, M64, 0x8000000000000000, 0xFFFFFFFF00000000, int(r.integers(0, 1 << 64, dtype=np.uint64))]
        bits = list(range(64)) + [64, 70, 127]  # the low 5 (32-bit forms) / 6 (64-bit form) bits of the index count: 32, 37, 63 and 64, 70, 127 wrap
        combos = [(v, b) for v in vals for b in bits]
        block, waves = 1024, 16
        G = -(-len(combos) // waves)
        while len(combos) < G * waves: combos.append((int(r.integers(0, 1 << 64, dtype=np.uint64)), int(r.integers(0, 128))))
        want = [(int((v & M32) != 0), (v & M32) & ~(1 << (b & 31)), (v & M32) | (1 << (b & 31)), v & ~(1 << (b & 63))) for v, b in combos]
        inp = np.repeat(np.array(combos, dtype=U64).reshape(G, waves, 1, 2), 64, axis=2)
        want = np.repeat(np.array(want, dtype=U64).reshape(G, waves, 1, 4), 64, axis=2)
        yield Launch("scalar_bits", G, block, inp, G * block * 4, lambda out: same_words(out, want, "nonzero01 / bit_clear / bit_set (per thread: nonzero01, bit_clear 32, bit_set 32, bit_clear 64; wavefront i holds combination i)"))
    return case


def _lds_ops(block):
    def case():
        r = _rng(14, block)
        G = 4
        a, b, c, v = (r.integers(0, 1 << 64, (G, block), dtype=np.uint64) for _ in range(4))
        x = (a ^ b) | c
        first = np.repeat(v[:, ::64], 64, axis=1)  # lane 0's value
        lane = np.arange(block) % 64
        want = np.stack([a, x, x ^ a, first, first, np.where(lane == 0, U64(M64), v)], axis=2)
        yield Launch("lds_ops", G, block, np.stack([a, b, c, v], axis=2), G * block * 6,
                     lambda out: same_words(out, want, f"lds_xor / lds_or / kfl_write / kfl_read block {block} (per thread: old of xor, old of the second xor, the word; kfl_read, the word, the dummy slot)"))
    return case


def _atomics():
    def case():
        r = _rng(15)
        G, block = 8, 1024
        val = r.integers(-(1 << 15), 1 << 15, G * block)
        adr = r.integers(0, 4, G * block)
        bits = r.integers(0, 1 << 64, G * block, dtype=np.uint64) & r.integers(0, 1 << 64, G * block, dtype=np.uint64) & r.integers(0, 1 << 64, G * block, dtype=np.uint64)
        bits &= U64(M64 ^ (1 << 40) ^ (1 << 3))  # two bits nobody sets
        preset = np.zeros((4, 7), U64); want = np.zeros((4, 7), U64)
        preset[:, 2] = 0x7FFFFFFF; preset[:, 3] = 0x80000000
        for k in range(4):
            sel = adr == k
            vs = [int(x) for x in val[sel]]
            ored = 0
            for x in bits[sel].tolist(): ored |= x
            want[k] = [int(np.float64(sum(vs)).view(U64)), sum(vs) & M32, min(vs) & M32, max(vs) & M32, sum(x & M32 for x in vs) & M64, ored, (ored >> 17) & M32]
        inp = np.stack([_i2w(val), adr.astype(U64), bits], axis=1)
        yield Launch("atomics", G, block, inp, 28, lambda out: same_words(out, want, "atomic_add f64 / atomic_add, min, max i32 / atomic_add, or u64 / atomic_or32: 8 192 threads into four addresses (seven words per address)"), preset=preset)
    return case


def _div_small():
    def case():
        a, b = np.meshgrid(np.arange(1025), np.arange(1, 65), indexing="ij")  # exhaustive: every pair the two functions are specified for
        a, b = a.reshape(-1), b.reshape(-1)
        n = a.size
        assert n == 65600
        block = 1024
        G = -(-n // block)
        want = np.stack([a // b, np.where(b <= 8, a // b, 0)], axis=1)

        def check(out):
            got = _w2i(out).reshape(n, 2)
            for col, name in ((0, "bk_div_small"), (1, "kfl_div")):
                bad = np.nonzero(got[:, col] != want[:, col])[0]
                assert bad.size == 0, f"{name}: {bad.size} of {n} quotients differ from a // b, first {int(a[bad[0]])} / {int(b[bad[0]])} = {int(got[bad[0], col])}"
        yield Launch("div_small", G, block, np.stack([_i2w(a), _i2w(b)], axis=1), n * 2, check)
    return case


def _kfl_table():
    def case():
        lv = np.repeat(np.arange(1, 9), 64)
        lane = np.tile(np.arange(64), 8)
        want = np.zeros((512, 10), U64)
        for i in range(512):
            want[i, 0] = sum((g // (int(lane[i]) + 1)) << (4 * (g - 1)) for g in range(1, int(lv[i]) + 1))
            for g in range(0, int(lv[i]) + 1): want[i, 1 + g] = g // (int(lane[i]) + 1)
        yield Launch("kfl_table", 8, 64, lv.astype(U64), 512 * 10, lambda out: same_words(out, want, "kfl_tab / kfl_quot (workgroup i: LV = i + 1; per thread: the table, the quotients for g = 0 .. 8)"))
    return case


def _all_cases():
    c = {}
    for b in BLOCKS + (100, 1): c[f"scan_int-b{b}"] = _scan_int(b)
    for b in BLOCKS:
        c[f"scan_f64_exact-b{b}"] = _scan_f64_exact(b)
        c[f"wave_max-b{b}"] = _wave_max(b)
    for b in (64, 256):
        c[f"scan_f64_rounding-b{b}"] = _scan_f64_rounding(b)
        c[f"key_scan-b{b}"] = _key_scan(b)
        c[f"lane_ops-b{b}"] = _lane_ops(b)
    for b in (64, 128, 1024):
        c[f"block_add3-b{b}"] = _block_add(3, b)
        c[f"block_add6-b{b}"] = _block_add(6, b)
        c[f"block_max-b{b}"] = _block_keys("block_max", b)
        c[f"block_excl-b{b}"] = _block_keys("block_excl", b)
    for b in (256, 100, 1, 1024): c[f"wg_scan-b{b}"] = _wg_scan(b)
    for b in (128, 1024): c[f"plan_setup-b{b}"] = _plan_setup(b)
    for b in (64, 256, 100, 1):
        c[f"shfl-b{b}"] = _shfl(b)
        c[f"ballot_rank-b{b}"] = _ballot_rank(b)
    c["scalar_bits"] = _scalar_bits()
    for b in (64, 1024): c[f"lds_ops-b{b}"] = _lds_ops(b)
    c["atomics"] = _atomics()
    c["div_small"] = _div_small()
    c["kfl_table"] = _kfl_table()
    return c


CASES = _all_cases()
