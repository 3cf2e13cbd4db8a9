"""EAM class-message kernels (csrc/eam_pool.hip) at the three levels of a 96^3 patch: 12^3 x 128, 24^3 x 64, 48^3 x 32,
nt = 16, fp32 and bf16 features. GPU time per call of u3d_eam_pool_fwd (tile kernel + combine) and u3d_eam_pool_bwd
(tile kernel + two combines, both gradients present), the way tools/kbench.py times a kernel: 20 calls captured in one
hipGraph and replayed three times between two device events (the capture is also the check that the entry points do
not synchronise with the host). Beside each time: the bytes of the feature x and the bandwidth they amount to (the
backward also writes dx: twice the bytes). Usage: python tools/bench_eam_pool.py [--out FILE]; one JSON line."""
import argparse
import json
import os
import sys

sys.path[:0] = [os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "multimodal-pl_amd")]
import torch  # noqa: E402
from u3d import ops  # noqa: E402
from u3d._lib import call, query  # noqa: E402

HEADS, NT = 4, 16


def t_(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(3):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (3 * reps) * 1e3


def level(s, c, dtype, dev):
    v, rows = s ** 3, HEADS * NT
    scale = (c // HEADS) ** -0.5
    x = torch.randn(v, c, device=dev).to(dtype)
    g2, b2 = torch.rand(c, device=dev) + 0.5, torch.randn(c, device=dev) * 0.1
    A = torch.randn(rows, c, device=dev) * (2.0 / (scale * c ** 0.5))
    new = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)   # noqa: E731
    att, yhat, stat = new(NT, v), new(rows, c), new(2 * rows)
    part = new(query("u3d_eam_pool_part_floats", v, c, NT))
    dy, gatt = torch.randn(rows, c, device=dev), torch.randn(NT, v, device=dev)
    dx, dA, dg2, db2 = torch.empty_like(x), new(rows, c), new(c), new(c)
    code = ops.dt_code(dtype)

    def fwd():
        call("u3d_eam_pool_fwd", code, x.data_ptr(), 1, v, c, g2.data_ptr(), b2.data_ptr(), A.data_ptr(), NT, HEADS,
             scale, att.data_ptr(), yhat.data_ptr(), stat.data_ptr(), part.data_ptr(), ops._stream())

    fwd()
    dd = (dy * yhat).sum(1)

    def bwd():
        call("u3d_eam_pool_bwd", code, x.data_ptr(), 1, v, c, g2.data_ptr(), b2.data_ptr(), A.data_ptr(), NT, HEADS,
             scale, stat.data_ptr(), dy.data_ptr(), dd.data_ptr(), gatt.data_ptr(), dx.data_ptr(), 0, part.data_ptr(),
             dA.data_ptr(), dg2.data_ptr(), db2.data_ptr(), 0, ops._stream())

    xb = x.numel() * x.element_size()
    f_us, b_us = t_(fwd), t_(bwd)
    return {"level": f"{s}^3 x {c}", "dtype": str(dtype).replace("torch.", ""), "x_bytes": xb,
            "blocks": query("u3d_eam_pool_blocks", v), "fwd_us": f_us, "fwd_x_GBps": xb / f_us / 1e3,
            "bwd_us": b_us, "bwd_x_dx_GBps": 2 * xb / b_us / 1e3}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=None)
    a = p.parse_args()
    dev = torch.device("cuda:0")
    rows = [level(s, c, dt, dev) for s, c in ((12, 128), (24, 64), (48, 32)) for dt in (torch.float32, torch.bfloat16)]
    line = json.dumps({"metric": "u3d_eam_pool_fwd / _bwd, us per call (hipGraph replay between device events)",
                       "nt": NT, "heads": HEADS, "levels": rows})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
