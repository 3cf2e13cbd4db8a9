"""The weight path kernel by kernel against the fp64 references of ws_reference.py: standardise + pack
(wstd_stats_kernel / wstd_pack_kernel of csrc/wprep.hip, u3d_wstd_fwd of csrc/wstd.hip), the split-K slab sum
(wstd_sum_slabs_kernel) and the standardisation backward (wstd_grad_row_kernel<4|8|16|28|56>, wstd_grad_kernel, the
single-conv wstd_bwd_kernel). The C entry points are called through u3d._lib, as u3d.ops calls them, on buffers the
test allocates itself and pre-fills with NaN, so an element the kernel leaves out cannot pass.

The bounds are worst-case counts of the fp32 roundings in the code (u = 2^-24), not measured figures:

  mean      |mean - ref| <= 2u |ref| + 1e-12 mean|w|          (fp64 sum, rounded once, one division)
  sd        |sd - ref|   <= 4u ref
  fp32 pack |pf - W^|    <= u (8 |W^| + 2 |mean| / sd)
  bf16 pack bitwise the .to(bfloat16) of the fp32 pack of the same entry point (both instantiate one fp32 expression),
            so |pf - W^| <= 2^-8 |W^| + the fp32 bound, which a half-spacing rounding just above a power of two reaches by design
  dgrad pack bitwise the transpose of the forward pack
  dW        |dW - ref|   <= u / sd [6 (|G_i| + |F1| + |W^_i F2|) + m (A1 / K + |W^_i| A2 / (K - 1))] + u |prev_i|
            m - 4 = the longest per-thread fp32 chain: ceil(K / 256) in the row kernel and in the single-conv kernel
            (whose sums are fp64), ceil(K / 64) in the chunked kernel; the single-conv path adds its fp32 slab tree,
            ns u sum_s |slab_s| / sd. Without standardisation: u |G_i| plus the slab term, and when accumulating
            u |prev_i + G_i| for the add in place of u |prev_i| (the add rounds its whole result).
  slab sum  |slab0 - ref| <= u |ref| + ns 2^-52 sum_s |slab_s|  (an fp64 sum, rounded once)

Every test prints its worst error as a share of the bound ("SHARE <family> <value>") before asserting.
"""
import ctypes
import functools
import math

import pytest
import torch

from ws_reference import LONG, ROW_MAX_K, SHAPES, U, pack_fwd, round32, unpack, ws_bwd_ref, ws_ref

pytestmark = pytest.mark.gpu

PAD = 777.0            # what the padding of the test's slabs holds: no kernel may let it reach dW
BATCH50 = [SHAPES[(0, 1, 2, 3, 4, 5, 6, 10, 11, 12)[i % 10]] for i in range(50)]  # > U3D_WSTD_BATCH_MAX = 48 descriptors
BATCHES = {"alone-" + "x".join(map(str, s)): [s] for s in SHAPES}
BATCHES.update({"all-but-long": [s for s in SHAPES if s != LONG],   # maxk = 8640: NPT 56 for the stem as well
                "all": list(SHAPES),                                # the long row sends every member to the chunked kernel
                "fifty": BATCH50})
MISALIGNED = [(24, 40, 3, True), (32, 32, 3, True), (64, 64, 1, True), (32, 1, 3, True)]


def _share(name, err, bound):
    """max err / bound (an entry with a zero bound must have no error); printed, then returned for the assertion."""
    assert bool(torch.isfinite(err).all()), name
    zero = bound == 0
    assert not bool((err[zero] != 0).any()), f"{name}: error where the bound is 0"
    s = (err[~zero] / bound[~zero]).max().item() if bool((~zero).any()) else 0.0
    print(f"SHARE {name} {s:.4f}")
    return s


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs and fp64 references of one shape, built once on the CPU and never modified."""
    cout, cin, k, std = shape
    gen = torch.Generator().manual_seed(100 * cout + 10 * cin + k)
    w = 0.1 * torch.randn(cout, cin, k, k, k, generator=gen) + 0.02
    col = (cout, 1, 1, 1, 1)
    if std:
        wh, mean, sd = ws_ref(w)
    else:
        wh, mean, sd = w.double(), torch.zeros(cout, dtype=torch.float64), torch.ones(cout, dtype=torch.float64)
    g = (0.7 * wh + 0.3 + 0.5 * torch.randn(w.shape, generator=gen)).float()
    ns = 1 + SHAPES.index(shape) % 4                       # 1..4 slabs; the slab counts have their own test
    wts = torch.rand((ns,) + w.shape, generator=gen) + 0.1
    parts = (g[None] * (wts / wts.sum(0))).float()         # random fp32 parts of g
    slabs = torch.stack([pack_fwd(p, PAD) for p in parts])
    G = unpack(slabs.double().sum(0), w.shape)             # the fp64 sum of those very slabs
    sabs = unpack(slabs.double().abs().sum(0), w.shape)
    prev = torch.randn(w.shape, generator=gen)
    return dict(shape=shape, w=w, wh=wh, mean=mean, sd=sd, col=col, ns=ns, slabs=slabs, G=G, sabs=sabs, prev=prev,
                bwd=ws_bwd_ref(w, G, std), K=cin * k ** 3)


# ------------------------------------------------------------------------------------------------ launchers
def _lib():
    from u3d import _lib as L
    return L


def _stream():
    from u3d.ops import _stream as s
    return s()


def _p(t):
    return None if t is None else t.data_ptr()


def _nan(shape, dtype, dev):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def _fwd_bufs(shape, dtype, dgrad, dev):
    cout, cin, k, std = shape
    k3, cp, cip = k ** 3, round32(cout), round32(cin)
    return (_nan((k3, cp, cip), dtype, dev), _nan((k3, cip, cp), dtype, dev) if dgrad else None,
            _nan((cout, 2), torch.float32, dev) if std else None)


def _fwd_batch(shapes, ws, dtype, dgrad, dev):
    """u3d_wstd_fwd_batch over (shape, device weight) pairs, 48 descriptors per call. Returns [(pf, pd, st)]."""
    L = _lib()
    out = [_fwd_bufs(s, dtype, dgrad, dev) for s in shapes]
    descs = [L.WstdDesc(w.data_ptr(), pf.data_ptr(), _p(pd), _p(st), None, None, s[0], s[1], s[2], int(s[3]), 1, 0)
             for s, w, (pf, pd, st) in zip(shapes, ws, out)]
    for i in range(0, len(descs), L.WSTD_BATCH_MAX):
        chunk = descs[i:i + L.WSTD_BATCH_MAX]
        arr = (L.WstdDesc * len(chunk))(*chunk)
        L.call("u3d_wstd_fwd_batch", L.BF16 if dtype == torch.bfloat16 else L.F32, ctypes.addressof(arr), len(chunk),
               _stream())
    return out


def _fwd_single(shape, w, dtype, dgrad, dev):
    L = _lib()
    pf, pd, st = _fwd_bufs(shape, dtype, dgrad, dev)
    L.call("u3d_wstd_fwd", L.BF16 if dtype == torch.bfloat16 else L.F32, w.data_ptr(), shape[0], shape[1], shape[2],
           int(shape[3]), pf.data_ptr(), _p(pd), _p(st), _stream())
    return pf, pd, st


def _bwd_batch(items):
    """u3d_wstd_bwd_batch over (shape, w, st, slabs, ns, dw, acc), 48 descriptors per call."""
    L = _lib()
    descs = [L.WstdDesc(w.data_ptr(), None, None, _p(st), part.data_ptr(), dw.data_ptr(), s[0], s[1], s[2], int(s[3]),
                        ns, int(acc)) for s, w, st, part, ns, dw, acc in items]
    scratch = torch.zeros(256, dtype=torch.uint8, device=items[0][1].device)
    for i in range(0, len(descs), L.WSTD_BATCH_MAX):
        chunk = descs[i:i + L.WSTD_BATCH_MAX]
        arr = (L.WstdDesc * len(chunk))(*chunk)
        assert L.query("u3d_wstd_bwd_scratch_bytes", ctypes.addressof(arr), len(chunk)) <= scratch.numel()
        L.call("u3d_wstd_bwd_batch", ctypes.addressof(arr), len(chunk), scratch.data_ptr(), _stream())


def _bwd_single(shape, w, st, part, ns, dw, acc):
    _lib().call("u3d_wstd_bwd", part.data_ptr(), ns, w.data_ptr(), _p(st), shape[0], shape[1], shape[2], int(shape[3]),
                dw.data_ptr(), int(acc), _stream())


# ------------------------------------------------------------------------------------------------ checks
def _check_fwd(tag, c, f32, bf):
    """f32, bf: (pf, pd, st) of one entry point in fp32 and in bf16."""
    cout, cin, k, std = c["shape"]
    torch.cuda.synchronize()
    pf, pd, st = (None if t is None else t.cpu() for t in f32)
    pfb, pdb, stb = (None if t is None else t.cpu() for t in bf)
    for t in (pf, pd, st, pfb, pdb, stb):
        assert t is None or bool(torch.isfinite(t).all()), f"{tag}: an element was not written"
    for t in (pf, pfb):                                      # the padding of both packs is exactly 0
        assert not t[:, cout:].any() and not t[:, :, cin:].any(), f"{tag}: forward pack padding"
    for t in (pd, pdb):
        assert t is None or (not t[:, cin:].any() and not t[:, :, cout:].any()), f"{tag}: dgrad pack padding"
    if std:
        for s in (st, stb):
            mean, sd = s[:, 0].double(), s[:, 1].double()
            bm = 2 * U * c["mean"].abs() + 1e-12 * c["w"].double().reshape(cout, -1).abs().mean(1)
            assert _share(f"mean {tag}", (mean - c["mean"]).abs(), bm) <= 1
            assert _share(f"sd {tag}", (sd - c["sd"]).abs(), 4 * U * c["sd"]) <= 1
        assert torch.equal(st, stb)
    else:
        assert st is None and stb is None
    wh = c["wh"]
    b32 = U * (8 * wh.abs() + 2 * (c["mean"].abs() / c["sd"]).reshape(c["col"]))
    assert _share(f"pack32 {tag}", (unpack(pf, wh.shape).double() - wh).abs(), b32) <= 1
    assert torch.equal(pfb.view(torch.int16), pf.to(torch.bfloat16).view(torch.int16)), f"{tag}: bf16 pack bits"
    assert _share(f"packbf {tag}", (unpack(pfb, wh.shape).double() - wh).abs(), 2.0 ** -8 * wh.abs() + b32) <= 1
    if pd is not None:
        assert torch.equal(pd, pf.transpose(1, 2)) and torch.equal(pdb, pfb.transpose(1, 2)), f"{tag}: dgrad pack"


def _bwd_bound(c, m, prev, slab_tree):
    ref = c["bwd"]
    K, sd, wh = c["K"], c["sd"].reshape(c["col"]), c["wh"]
    G = c["G"].abs()
    if c["shape"][3]:
        b = U / sd * (6 * (G + ref.F1.abs() + (wh * ref.F2).abs()) + m * (ref.A1 / K + wh.abs() * ref.A2 / (K - 1)))
        if prev is not None:
            b = b + U * prev.double().abs()
    else:
        # dW = fl(prev + fl(G)): the rounding of the sum, u |G|, then one fp32 add, u |prev + fl(G)|. The add rounds the
        # G part as well, so u |prev| alone is not a bound there (measured 1.30 of it at (8, 32, 1)); with the
        # standardisation the 6 u |G| / sd above covers that part.
        b = U * G
        if prev is not None:
            b = b + U * (1 + 2 * U) * (prev.double() + c["G"]).abs()
    if slab_tree:
        b = b + c["ns"] * U * c["sabs"] / sd
    return b


def _check_bwd(tag, c, dw, kernel, prev, slab_tree=False):
    chain = math.ceil(c["K"] / (64 if kernel == "chunk" else 256))
    want = c["bwd"].dw + (prev.double() if prev is not None else 0)
    got = dw.cpu()
    assert bool(torch.isfinite(got).all()), f"{tag}: an element was not written"
    fam = f"bwd-{kernel}" + ("" if c["shape"][3] else "-unstd")
    assert _share(f"{fam} {tag}", (got.double() - want).abs(), _bwd_bound(c, chain + 4, prev, slab_tree)) <= 1


@functools.lru_cache(maxsize=None)
def _stats(shape, dev):
    """The fp32 (mean, sd) the forward hands the backward, from the batched forward (checked by the forward tests)."""
    if not shape[3]:
        return None
    return _fwd_batch([shape], [_case(shape)["w"].to(dev)], torch.float32, False, dev)[0][2]


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("dgrad", [False, True], ids=["nodgrad", "dgrad"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_fwd_single(gpu, shape, dgrad):
    c = _case(shape)
    w = c["w"].to(gpu)
    _check_fwd("single", c, _fwd_single(shape, w, torch.float32, dgrad, gpu),
               _fwd_single(shape, w, torch.bfloat16, dgrad, gpu))


@pytest.mark.parametrize("dgrad", [False, True], ids=["nodgrad", "dgrad"])
@pytest.mark.parametrize("batch", BATCHES, ids=str)
def test_fwd_batch(gpu, batch, dgrad):
    shapes = BATCHES[batch]
    ws = [_case(s)["w"].to(gpu) for s in shapes]
    f32 = _fwd_batch(shapes, ws, torch.float32, dgrad, gpu)
    bf = _fwd_batch(shapes, ws, torch.bfloat16, dgrad, gpu)
    for s, a, b in zip(shapes, f32, bf):
        _check_fwd("batch", _case(s), a, b)


# ------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("acc", [0, 1], ids=["write", "accumulate"])
@pytest.mark.parametrize("row", [1, 0], ids=["row", "chunked"])
@pytest.mark.parametrize("batch", BATCHES, ids=str)
def test_bwd_batch(gpu, batch, row, acc):
    from u3d import ops
    shapes = BATCHES[batch]
    kernel = "row" if row and max(_case(s)["K"] for s in shapes) <= ROW_MAX_K else "chunk"
    items = []
    for s in shapes:
        c = _case(s)
        dw = c["prev"].to(gpu) if acc else _nan(c["w"].shape, torch.float32, gpu)
        items.append((s, c["w"].to(gpu), _stats(s, gpu), c["slabs"].to(gpu), c["ns"], dw, acc))
    with ops.option("WSTD_ROW", row):
        _bwd_batch(items)
    torch.cuda.synchronize()
    for it in items:
        c = _case(it[0])
        _check_bwd("batch", c, it[5], kernel, c["prev"] if acc else None)
        # the batch leaves the fp64 sum of the slabs, rounded once, in slab 0
        ref = c["slabs"].double().sum(0)
        got = it[3][0].cpu().double()
        valid = pack_fwd(torch.ones(c["w"].shape), 0.0).bool()
        bound = U * ref.abs() + c["ns"] * 2.0 ** -52 * c["slabs"].double().abs().sum(0)
        assert _share("slabsum in-batch", (got - ref).abs()[valid], bound[valid]) <= 1


@pytest.mark.parametrize("acc", [0, 1], ids=["write", "accumulate"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_bwd_single(gpu, shape, acc):
    c = _case(shape)
    dw = c["prev"].to(gpu) if acc else _nan(c["w"].shape, torch.float32, gpu)
    _bwd_single(shape, c["w"].to(gpu), _stats(shape, gpu), c["slabs"].to(gpu), c["ns"], dw, acc)
    torch.cuda.synchronize()
    _check_bwd("single", c, dw, "single", c["prev"] if acc else None, slab_tree=True)


# ------------------------------------------------------------------------------------------------ slab sums
@functools.lru_cache(maxsize=None)
def _slabs(cout, cin, k, ns):
    gen = torch.Generator().manual_seed(7 * ns + k)
    s = torch.randn((ns, k ** 3, round32(cout), round32(cin)), generator=gen)
    d = s.double()
    return s, d.sum(0), d.abs().sum(0)


SLAB_CASES = [(32, 32, k, ns) for k in (1, 3) for ns in (1, 2, 8, 9, 16, 17, 33, 100, 257, 600)] + \
             [(64, 256, 3, 2), (64, 256, 3, 9), (24, 40, 3, 9), (8, 544, 3, 3)]   # K >= 6912: ns <= 9


@pytest.mark.parametrize("entry", ["eager", "batch"])
@pytest.mark.parametrize("cout,cin,k,ns", SLAB_CASES, ids=str)
def test_slab_sum(gpu, cout, cin, k, ns, entry):
    """sg steps 1 -> 2 -> 4 -> ... -> 32 at ns = 17, 33, 65, ..., 257; ns in {9, 16, 17, 33, 100, 257} need a second round
    of 8 loads (ns > 8 sg), the last one partial with clamped addresses; ns = 600 a third. Contract: the sum lands in
    slab 0 and the kernel writes nothing else, so slabs 1..ns-1 stay bitwise as they were."""
    L = _lib()
    src, ref, sabs = _slabs(cout, cin, k, ns)
    part = src.to(gpu)
    if entry == "eager":
        L.call("u3d_wgrad_sum_slabs", part.data_ptr(), ns, k ** 3, cout, cin, _stream())
    else:
        w = torch.zeros((cout, cin, k, k, k), device=gpu)
        _bwd_batch([((cout, cin, k, False), w, None, part, ns, torch.empty_like(w), 0)])
    torch.cuda.synchronize()
    got = part.cpu()
    assert torch.equal(got[1:], src[1:]), "a slab other than 0 changed"
    assert _share(f"slabsum {entry}", (got[0].double() - ref).abs(), U * ref.abs() + ns * 2.0 ** -52 * sabs) <= 1


# ------------------------------------------------------------------------------------------------ misaligned operands
@pytest.mark.parametrize("off", [1, 2])
@pytest.mark.parametrize("shape", MISALIGNED, ids=str)
def test_misaligned(gpu, shape, off):
    """w and dw as views 1 and 2 floats into larger buffers, as the DDP bucket views sit (4-byte aligned only): the same
    bounds, and the floats either side of dw untouched."""
    from u3d import ops
    c = _case(shape)
    n = c["w"].numel()
    wbuf = torch.full((n + 8,), 1e30, device=gpu)
    w = wbuf[off:off + n].view(c["w"].shape)
    w.copy_(c["w"])
    assert w.data_ptr() % 16 == 4 * off
    for tag, run in (("single-misaligned", lambda dt: _fwd_single(shape, w, dt, True, gpu)),
                     ("batch-misaligned", lambda dt: _fwd_batch([shape], [w], dt, True, gpu)[0])):
        f32 = run(torch.float32)
        _check_fwd(tag, c, f32, run(torch.bfloat16))
    st = f32[2]
    for kernel, acc in [(kn, a) for kn in ("row", "chunk", "single") for a in (0, 1)]:
        dbuf = torch.full((n + 8,), -12345.0, device=gpu)
        dw = dbuf[off:off + n].view(c["w"].shape)
        dw.copy_(c["prev"]) if acc else dw.fill_(float("nan"))
        part = c["slabs"].to(gpu)
        if kernel == "single":
            _bwd_single(shape, w, st, part, c["ns"], dw, acc)
        else:
            with ops.option("WSTD_ROW", int(kernel == "row")):
                _bwd_batch([(shape, w, st, part, c["ns"], dw, acc)])
        torch.cuda.synchronize()
        _check_bwd("misaligned", c, dw, kernel, c["prev"] if acc else None, slab_tree=kernel == "single")
        assert bool((dbuf[:off] == -12345.0).all()) and bool((dbuf[off + n:] == -12345.0).all()), "dw sentinels"
    assert bool((wbuf[:off] == 1e30).all()) and bool((wbuf[off + n:] == 1e30).all())
