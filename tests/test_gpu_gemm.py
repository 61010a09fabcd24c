"""GEMM paths at their tile edges, against the fp64 oracles of gemm_check.py.

Every test forces its kernel path with nvit_set_gemm_impl / nvit_set_gemm_sched (process-global switches, restored
in `finally`):
  * NT 128x128 kernel (nt_impl 0); NT persistent 256x128 (nt_impl 2, N % 256 != 0) and 256x256 (N % 256 == 0) with the
    LDS-staged epilogue, and with the direct epilogue (EPI 0: N or ldc not a multiple of 16 B of output);
  * NT 256x256 with dynamic tile scheduling (sched 1), bitwise against static, and the fused SwiGLU / SwiGLU-backward /
    q-k-normalise GEMMs under both schedules;
  * TN 128x128 kernel (tn_impl 0) and persistent 256x256 kernel (tn_impl 1), with the library's split counts and with
    explicit ones into a workspace pre-filled with NaN.
Operands are views inside larger buffers whose padding (columns past K / N, rows past M / Mred) is NaN: a NaN in a
result means a kernel summed memory it must not read.  Outputs are views inside buffers filled with a sentinel bit
pattern that must be unchanged afterwards.  Exact (integer) data must come out bit-exact; fp32 operands also run on
Gaussian data against the probabilistic bound, whose margin max(err / bound) is printed (-s)."""
import contextlib

import pytest
import torch

import gemm_check as gc

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTS = [F32, BF16]
DT_ID = {F32: "f32", BF16: "bf16"}
SENTINEL = {F32: 0x7FA5A5A5, BF16: 0x7FA5}         # NaN bit patterns (outputs written without "+=")
SENTINEL_FINITE = {F32: 0x4B3C614E, BF16: 0x4B3C}   # finite (accumulate cases)


def dev():
    return torch.device("cuda:0")


def ops_():
    from nvit_amd import ops
    return ops


def lib():
    from nvit_amd import _lib
    return _lib.load()


def _check(rc, what):
    from nvit_amd._lib import check
    check(rc, what)


@contextlib.contextmanager
def paths(nt=-1, tn=-1, sched=0):
    """Force the GEMM kernel paths; the defaults are restored even when the body fails."""
    try:
        _check(lib().nvit_set_gemm_impl(nt, tn), "nvit_set_gemm_impl")
        _check(lib().nvit_set_gemm_sched(sched), "nvit_set_gemm_sched")
        yield
    finally:
        lib().nvit_set_gemm_impl(-1, -1)
        lib().nvit_set_gemm_sched(0)


def unit(dtype):
    return 16 // torch.empty((), dtype=dtype).element_size()


def _bits(t):
    return t.view(torch.int32) if t.dtype == F32 else t.view(torch.int16)


def place(x, dtype, col_off=0, rows_pad=5):
    """x (CPU) as a view [R, C] inside a NaN-filled device buffer: col_off columns before it (16-byte aligned), one
    16-byte chunk after it (ld > C), rows_pad rows below it."""
    R, Cc = x.shape
    buf = torch.full((R + rows_pad, col_off + Cc + unit(dtype)), float("nan"), dtype=dtype, device=dev())
    view = buf[:R, col_off:col_off + Cc]
    view.copy_(x.to(dtype))
    return view


class Out:
    """An output view [M, N] inside a sentinel-filled buffer (ld = `ld`, or N + one chunk + col_off)."""

    def __init__(self, M, N, dtype, ld=None, col_off=0, finite=False, init=None):
        width = ld if ld is not None else col_off + N + unit(dtype)
        assert col_off + N <= width and col_off % unit(dtype) == 0
        self.buf = torch.empty((M + 3, width), dtype=dtype, device=dev())
        _bits(self.buf).fill_((SENTINEL_FINITE if finite else SENTINEL)[dtype])
        self.view = self.buf[:M, col_off:col_off + N]
        if init is not None:
            self.view.copy_(init.to(dtype))
        self.mask = torch.ones(self.buf.shape, dtype=torch.bool, device=dev())
        self.mask[:M, col_off:col_off + N] = False
        self.before = self.buf.clone()

    def assert_guard(self, label):
        torch.cuda.synchronize()
        ok = torch.equal(_bits(self.buf)[self.mask], _bits(self.before)[self.mask])
        assert ok, f"{label}: wrote outside its output view"


def _dv(t):
    return None if t is None else t.to(dev())


# ---------------------------------------------------------------------------------------------------- NT
def run_nt(dtype, M, N, K, out_dtype, *, data="exact", bias=False, colscale=False, period=0, accumulate=False,
           cancel=False, ld=None, a_off=0, c_off=0, seed=0, tag=""):
    """One nvit_gemm_nt call through the currently forced path, checked against the fp64 reference (exact data:
    bit-exact; Gaussian: the bound).  Returns the Gaussian margin (0 for exact data)."""
    exact = data == "exact"
    if exact:
        old_amax = (K * 16 * 1.1 + 64) if accumulate else 0.0
        d = gc.nt_exact(M, N, K, seed, bias=bias, colscale=colscale, period=period, old_amax=old_amax)
    else:
        d = {"A": gc.gauss_data((M, K), seed), "B": gc.gauss_data((N, K), seed + 1),
             "bias": gc.gauss_data((N,), seed + 2) if bias else None,
             "colscale": gc.gauss_data((N,), seed + 3) if colscale else None,
             "rowadd": gc.gauss_data((period, N), seed + 4) if period else None}
    A, B = d["A"].to(dtype), d["B"].to(dtype)   # what the kernel sees
    bias_, cs, radd = d["bias"], d["colscale"], d["rowadd"]
    rows = gc.sample_rows(M)
    old = None
    if accumulate:
        if cancel:
            assert rows is None
            ref0, _ = gc.nt_ref(A, B, None, bias_, cs, radd, period)
            old = gc.cancelling_old(ref0, seed + 5) if exact else (-ref0 * (1 + 2.0 ** -5 * gc.gauss_data(ref0.shape,
                                                                                                          seed + 5)))
        else:
            old = gc.int_data((M, N), 64, seed + 5) if exact else gc.gauss_data((M, N), seed + 5)
        old = old.to(out_dtype)                  # the value the kernel reads back
    Av = place(A, dtype, col_off=a_off)
    Bv = place(B, dtype)
    out = Out(M, N, out_dtype, ld=ld, col_off=c_off, finite=accumulate, init=old)
    ops_().gemm_nt(Av, Bv, M, N, K, out=out.view, bias=_dv(bias_), colscale=_dv(cs), rowadd=_dv(radd),
                   rowadd_period=period, accumulate=accumulate)
    label = (f"nt{tag} {DT_ID[dtype]}->{DT_ID[out_dtype]} M{M} N{N} K{K} ld{out.view.stride(0)}"
             f"{' bias' if bias else ''}{' cs' if colscale else ''}{f' rowadd%{period}' if period else ''}"
             f"{' +=' if accumulate else ''}{' cancel' if cancel else ''} {data}")
    out.assert_guard(label)
    got = out.view.cpu() if rows is None else out.view[rows.to(dev())].cpu()
    oldr = None if old is None else (old.float() if rows is None else old.float()[rows])
    ref, mag = gc.nt_ref(A, B, rows, bias_, cs, radd, period, oldr)
    if exact:
        gc.assert_exact(got, ref, label)
        return 0.0
    return gc.check_gauss(got, ref, mag, K, label)


def run_nt_both(dtype, *args, **kw):
    """Exact data, and for fp32 operands Gaussian data as well."""
    run_nt(dtype, *args, **kw)
    if dtype == F32:
        run_nt(dtype, *args, data="gauss", **kw)


@pytest.mark.parametrize("out_dtype", DTS, ids=DT_ID.get)
@pytest.mark.parametrize("dtype", DTS, ids=DT_ID.get)
def test_nt_128_tile_edges(dtype, out_dtype):
    bk = 32 if dtype == F32 else 64
    ks = (bk, 2 * bk, 3 * bk, 768, 3072)
    i = 0
    with paths(nt=0):
        for M in (1, 127, 128, 129, 255):
            for N in (1, 10, 127, 129):
                run_nt_both(dtype, M, N, ks[i % 5], out_dtype, a_off=unit(dtype) * (i % 2),
                            c_off=unit(out_dtype) * (i % 3 == 0), seed=i, tag=" 128")
                i += 1


@pytest.mark.parametrize("out_dtype", DTS, ids=DT_ID.get)
@pytest.mark.parametrize("dtype", DTS, ids=DT_ID.get)
def test_nt_persistent_tile_edges(dtype, out_dtype):
    i = 0
    with paths(nt=2):
        for N, ks in (((128, 1032, 1000), (64, 128, 192, 256, 448)),       # 256x128 tiles (3-slot ring at K = 192)
                      ((256, 512), (64, 128, 384, 448, 3072))):            # 256x256 tiles
            for M in (1, 255, 256, 257, 511):
                for n in N:
                    run_nt_both(dtype, M, n, ks[i % 5], out_dtype, a_off=unit(dtype) * (i % 2),
                                c_off=unit(out_dtype) * (i % 3 == 0), seed=100 + i, tag=" p")
                    i += 1


@pytest.mark.parametrize("out_dtype", DTS, ids=DT_ID.get)
@pytest.mark.parametrize("dtype", DTS, ids=DT_ID.get)
def test_nt_persistent_direct_epilogue(dtype, out_dtype):
    """N or ldc not a multiple of 16 B of output: the persistent kernels store directly (EPI 0)."""
    with paths(nt=2):
        for j, (M, N, ld) in enumerate(((255, 1001, None), (257, 1004, None), (511, 1000, 1002), (257, 1001, 1001))):
            run_nt_both(dtype, M, N, 192, out_dtype, ld=ld, bias=True, colscale=True, period=7, seed=200 + j,
                        tag=" p-direct")
            run_nt_both(dtype, M, N, 128, out_dtype, ld=ld, accumulate=True, seed=210 + j, tag=" p-direct")


EPI_PATHS = {"128": (0, 255, 136, 192), "p256x128": (2, 257, 1000, 192), "p256x256": (2, 257, 512, 448),
             "p-direct": (2, 257, 1001, 192)}


@pytest.mark.parametrize("path", list(EPI_PATHS))
@pytest.mark.parametrize("out_dtype", DTS, ids=DT_ID.get)
@pytest.mark.parametrize("dtype", DTS, ids=DT_ID.get)
def test_nt_epilogues(dtype, out_dtype, path):
    nt, M, N, K = EPI_PATHS[path]
    combos = [dict(bias=True), dict(colscale=True), dict(bias=True, colscale=True)]
    combos += [dict(bias=True, colscale=True, period=p) for p in (1, 7, 196, M)]
    combos += [dict(accumulate=True), dict(accumulate=True, cancel=True),
               dict(bias=True, colscale=True, period=7, accumulate=True)]
    with paths(nt=nt):
        for j, kw in enumerate(combos):
            run_nt_both(dtype, M, N, K, out_dtype, c_off=unit(out_dtype) * (j % 2), seed=300 + j, tag=" " + path, **kw)


def _dyn_operands(dtype, M, N, K, seed):
    d = gc.nt_exact(M, N, K, seed)
    return d["A"].to(dtype), d["B"].to(dtype)


@pytest.mark.parametrize("dtype", DTS, ids=DT_ID.get)
def test_nt_dynamic_schedule_bitwise(dtype):
    """Dynamic tile hand-out (256x256, more tiles than CUs, K/BK >= 6) gives the static result bit for bit; then 66
    dynamic launches of alternating shapes (the 64 scheduler slots wrap, each launch's last workgroup resets its slot),
    every one bitwise equal to its static result."""
    ops = ops_()
    out_dtype = dtype
    shapes = [(256 * 40 + 1, 2048, 512), (256 * 20 + 17, 4096, 384)]
    cases = []
    for s, (M, N, K) in enumerate(shapes):
        A, B = _dyn_operands(dtype, M, N, K, 400 + s)
        Av, Bv = place(A, dtype), place(B, dtype)
        with paths(nt=2, sched=0):
            ref_out = ops.gemm_nt(Av, Bv, M, N, K, out_dtype=out_dtype)
        torch.cuda.synchronize()
        rows = gc.sample_rows(M)
        ref, _ = gc.nt_ref(A, B, rows)
        gc.assert_exact(ref_out[rows.to(dev())].cpu(), ref, f"static M{M} N{N} K{K}")
        out = Out(M, N, out_dtype)
        cases.append((Av, Bv, M, N, K, ref_out, out))
    with paths(nt=2, sched=1):
        for it in range(66):
            Av, Bv, M, N, K, ref_out, out = cases[it % 2]
            _bits(out.view).fill_(SENTINEL[out_dtype])
            ops.gemm_nt(Av, Bv, M, N, K, out=out.view)
            torch.cuda.synchronize()
            assert gc.bits_equal(out.view, ref_out), f"dynamic launch {it} (M{M} N{N} K{K}) differs from static"
            if it < 2:
                out.assert_guard(f"dynamic M{M} N{N} K{K}")


def test_fused_gemms_dynamic_schedule_bitwise():
    """The fused-epilogue GEMMs at an M with a tail: dynamic scheduling bitwise equal to static."""
    ops = ops_()
    g = lambda shape, seed, s=1.0: (gc.gauss_data(shape, seed) * s)
    K, F = 768, 4096
    M = 5123
    assert ops.fusable(1, M, 2 * F, K) and ops.fusable(1, M, F, K)
    A = g((M, K), 500).to(BF16).to(dev())
    Bsw = g((2 * F, K), 501, 0.05).to(BF16).to(dev())
    Bbw = g((F, K), 502, 0.05).to(BF16).to(dev())
    gs = (1 + 0.1 * g((2 * F,), 503)).to(dev())
    res = {}
    for sched in (0, 1):
        with paths(nt=-1, sched=sched):
            uv, xm = ops.gemm_nt_swiglu(A, Bsw, M, F, K, gs, 1.5)
            duv, part = ops.gemm_nt_swiglu_bwd(A, Bbw, uv, M, F, K, gs, 1.5)
            torch.cuda.synchronize()
            res[sched] = {"uv": uv, "xm": xm, "duv": duv, "part": part}
    for k in res[0]:
        assert gc.bits_equal(res[0][k], res[1][k]), f"{k}: dynamic differs from static"
    assert torch.isfinite(res[0]["duv"].float()).all() and torch.isfinite(res[0]["xm"].float()).all()
    # q/k/v projection with the per-head normalise: T = 197 tokens, 52 images (M = 10244, a 4-row tail tile)
    T, Bsz, H, d = 197, 52, 12, 64
    C = H * d
    Mq = T * Bsz
    Aq = g((Mq, C), 504).to(BF16).to(dev())
    Bq = g((3 * C, C), 505, 0.05).to(BF16).to(dev())
    sqk = (1 + 0.1 * g((C,), 506)).to(dev())
    outs = {}
    for sched in (0, 1):
        with paths(nt=-1, sched=sched):
            outs[sched] = ops.gemm_nt_qknorm(Aq, Bq, Mq, C, 3, 0, sqk, 2.0, Bsz, T, H, d,
                                             q_prescale=ops.attn_q_prescale(d))
            torch.cuda.synchronize()
    for name, a, b in zip(("qh", "kh", "vh", "rq", "rk"), outs[0], outs[1]):
        assert gc.bits_equal(a, b), f"qknorm {name}: dynamic differs from static"


# ---------------------------------------------------------------------------------------------------- TN
def run_tn(dtype, Mred, N, K, *, data="exact", perm=0, accumulate=False, splits=None, seed=0, tag="", repeat=False):
    """One nvit_gemm_tn call (the library's split count, or `splits` explicitly into a NaN-filled workspace) through
    the currently forced path.  Rows after Mred and columns after N / K of the operands are NaN."""
    ops = ops_()
    exact = data == "exact"
    if exact:
        d = gc.tn_exact(Mred, N, K, seed, old_amax=64 if accumulate else 0)
        old = gc.int_data((N, K), 64, seed + 2) if accumulate else None
    else:
        d = {"A": gc.gauss_data((Mred, N), seed), "B": gc.gauss_data((Mred, K), seed + 1)}
        old = gc.gauss_data((N, K), seed + 2) if accumulate else None
    A, B = d["A"].to(dtype), d["B"].to(dtype)
    Av = place(A, dtype, col_off=unit(dtype) * (seed % 2))
    Bv = place(B, dtype)
    out = Out(N, K, F32, col_off=4 * (seed % 3 == 0), finite=accumulate, init=old)
    dt = 0 if dtype == F32 else 1

    def call(G):
        if splits is None:
            ops.gemm_tn(Av, Bv, G, Mred, N, K, perm=perm, accumulate=accumulate)
            return ops.tn_splits(Mred, N, K, dt)
        ws = torch.full((splits * N * K + 64,), float("nan"), device=dev())
        _check(lib().nvit_gemm_tn(dt, Av.data_ptr(), Av.stride(0), Bv.data_ptr(), Bv.stride(0), G.data_ptr(),
                                  G.stride(0), Mred, N, K, splits, ws.data_ptr(), ws.numel() * 4, perm,
                                  int(accumulate), torch.cuda.current_stream().cuda_stream), "nvit_gemm_tn")
        return splits

    ns = call(out.view)
    label = (f"tn{tag} {DT_ID[dtype]} Mred{Mred} N{N} K{K} ldg{out.view.stride(0)} splits{ns}"
             f"{' perm' if perm else ''}{' +=' if accumulate else ''} {data}")
    out.assert_guard(label)
    got = out.view.cpu()
    if repeat:   # documented deterministic: a second call gives the same bits
        again = Out(N, K, F32, finite=accumulate, init=old)
        call(again.view)
        torch.cuda.synchronize()
        assert gc.bits_equal(again.view.cpu(), got), f"{label}: two calls differ"
    ref, mag = gc.tn_ref(A, B, Mred, perm, None if old is None else old)
    if exact:
        gc.assert_exact(got, ref, label)
        return 0.0
    return gc.check_gauss(got, ref, mag, Mred + ns, label)


def run_tn_both(dtype, *args, **kw):
    run_tn(dtype, *args, **kw)
    if dtype == F32:
        run_tn(dtype, *args, data="gauss", **kw)


@pytest.mark.parametrize("dtype", DTS, ids=DT_ID.get)
def test_tn_128_edges(dtype):
    i = 0
    with paths(tn=0):
        for Mred in (1, 63, 64, 65, 130, 9001):
            for N, K in ((8, 8), (40, 136), (128, 40), (136, 128)):
                run_tn_both(dtype, Mred, N, K, accumulate=i % 3 == 1, seed=600 + i, tag=" 128")
                i += 1
        run_tn_both(dtype, 1000, 128, 136, perm=1, accumulate=True, seed=650, tag=" 128")


@pytest.mark.parametrize("dtype", DTS, ids=DT_ID.get)
def test_tn_persistent(dtype):
    i = 0
    with paths(tn=1):
        for Mred in (4095, 4096, 4097, 4159, 9001):     # 4095: below the persistent kernel's minimum, falls back
            for N, K in ((256, 256), (512, 256)):
                run_tn_both(dtype, Mred, N, K, accumulate=i % 2 == 1, seed=700 + i, tag=" p", repeat=i < 2)
                i += 1
        run_tn_both(dtype, 9001, 512, 256, perm=1, accumulate=True, seed=750, tag=" p")


@pytest.mark.parametrize("tn", [0, 1], ids=["tn128", "tn-persistent"])
@pytest.mark.parametrize("dtype", DTS, ids=DT_ID.get)
def test_tn_explicit_splits(dtype, tn):
    """Split counts that leave trailing splits empty (64-row rounding of rows_per_split): an empty split must still
    zero its slab of the NaN-filled workspace."""
    cases = [(4160, 256, 256, 64), (4160, 256, 256, 3), (4160, 256, 256, 1), (9001, 256, 512, 3), (9001, 256, 256, 64)]
    if tn == 0:
        cases += [(130, 136, 40, 64), (1000, 40, 128, 3), (65, 8, 8, 64)]
    with paths(tn=tn):
        for j, (Mred, N, K, s) in enumerate(cases):
            run_tn_both(dtype, Mred, N, K, splits=s, accumulate=j % 2 == 1, seed=800 + j, tag=f" {tn}",
                        repeat=True)
