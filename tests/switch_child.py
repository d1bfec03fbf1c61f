"""A helper of test_engine_switches_gpu.py, not a test: ONE process under one setting of the three variables the library reads
once per process (LKG_GEMM_F32_ONLY, LKG_ACTLN_NARROW_OFF, LKG_SMALLM_BLOCKS), started by the parent with the variable in its
environment.  It builds nothing (the parent's fixture has built the library), runs the three entry points the variables
steer through the C ABI, holds each to its float64 reference at the allowance the direct tests apply, and prints one JSON
line; an assertion that fails ends it with a non-zero status.

    lkg_gemm_f32            16461 x 256 . 256^T with the workspace lkg_gemm_workspace asks for, and A^T B with k = 4099,
                            256 x 128: the engine lkg_gemm_f32_engine reports, the error over the result's largest entry next
                            to torch's float32 product (the parent asserts engines and bounds: test_gpu_parity.py:253, :276)
    lkg_act_layernorm_fwd   n = 4099, d in (32, 64, 128), with and without yn: rowwise_cases.check_layernorm_fwd
    lkg_gemm_smallm_f32     32 x 32 and 64 x 96 at k = 4099 + 3 * 256: op_audit's smallm allowance; two runs compared bit for bit"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch

import op_audit as A
import rowwise_cases as C
from literalkg_amd import _native as N


def gemm_f32(dev, out):
    lib = N.load()
    gen = torch.Generator(device=dev).manual_seed(11)
    for name, ta, tb, m, n, k in (("rows", 0, 1, 16461, 256, 256), ("kmajor", 1, 0, 256, 128, 4099)):
        a = torch.randn((k, m) if ta else (m, k), device=dev, generator=gen)
        b = torch.randn((n, k) if tb else (k, n), device=dev, generator=gen) * 0.1
        need = int(lib.lkg_gemm_workspace(ta, m, n, k))
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
        got = torch.empty((m, n), device=dev)
        N.call("lkg_gemm_f32", ta, tb, m, n, k, 1.0, N.ptr(a), a.shape[1], N.ptr(b), b.shape[1], 0.0, N.ptr(got), n, None,
               N.ptr(ws) if need else None, need, None)
        torch.cuda.synchronize()
        a_, b_ = (a.t() if ta else a), (b.t() if tb else b)
        want = a_.double() @ b_.double()
        scale = float(want.abs().max())
        out[f"gemm_{name}"] = dict(engine=int(lib.lkg_gemm_f32_engine(ta, tb, m, n, k, need)), workspace=need,
                                   err=float((got.double() - want).abs().max()) / scale,
                                   f32=float(((a_ @ b_).double() - want).abs().max()) / scale)


def act_layernorm(dev, out):
    worst = 0.0
    for d in (32, 64, 128):
        for with_yn in (True, False):
            case = C.draw_layernorm(dev, 4099, d)
            n = case.n
            y = torch.full((n + 1, d), C.SENTINEL, device=dev)
            yn = torch.full((n + 1, d), C.SENTINEL, device=dev) if with_yn else None
            mean, rstd = torch.empty(n, device=dev), torch.empty(n, device=dev)
            N.call("lkg_act_layernorm_fwd_f32", n, d, N.ptr(case.z), d, case.slope, N.ptr(case.gamma), N.ptr(case.beta), case.eps,
                   N.ptr(y), d, N.ptr(yn), d if with_yn else 0, case.norm_eps, N.ptr(mean), N.ptr(rstd), 0.0, 0, None)
            torch.cuda.synchronize()
            for t in (y, yn):
                assert t is None or bool((t[n] == C.SENTINEL).all()), f"layernorm d {d}: the guard row was written"
            lines = []
            C.check_layernorm_fwd(lines, case, dict(mean=mean, rstd=rstd, y=y[:n], yn=yn[:n] if with_yn else None))
            worst = max([worst] + [r / b for _, r, b in lines if b])
    out["act_layernorm"] = dict(cases=6, worst_r_over_bound=worst)


def smallm(dev, out):
    gen = torch.Generator(device=dev).manual_seed(13)
    k = 4099 + 256 * 3
    res = {}
    for m, n in ((32, 32), (64, 96)):
        a = torch.randn(k, m, device=dev, generator=gen)
        b = torch.randn(k, n, device=dev, generator=gen)
        assert N.load().lkg_gemm_smallm_ok(m, n, k, N.ptr(a), m, N.ptr(b), n)
        runs = []
        for _ in range(2):
            got = torch.full((m + 1, n), C.SENTINEL, device=dev)
            N.call("lkg_gemm_smallm_f32", m, n, k, N.ptr(a), m, N.ptr(b), n, N.ptr(got), n, None)
            torch.cuda.synchronize()
            assert bool((got[m] == C.SENTINEL).all()), "smallm: the guard row was written"
            runs.append(got[:m])
        want = a.double().t() @ b.double()
        scale = a.double().abs().t() @ b.double().abs()
        r32 = A.componentwise(a.t() @ b, want, scale)[0]
        r = max(A.componentwise(g, want, scale)[0] for g in runs)
        bound = A.bound_for("smallm", r32, k)
        assert r <= bound, f"smallm {m} x {n}: r {r:.3g} > {bound:.3g} (torch f32 {r32:.3g})"
        res[f"{m}x{n}"] = dict(r=r, bound=bound, same_bits=bool(torch.equal(runs[0], runs[1])))
    out["smallm"] = res


def main():
    dev = torch.device("cuda:0")
    out = {"env": {k: os.environ[k] for k in ("LKG_GEMM_F32_ONLY", "LKG_ACTLN_NARROW_OFF", "LKG_SMALLM_BLOCKS") if k in os.environ}}
    gemm_f32(dev, out)
    act_layernorm(dev, out)
    smallm(dev, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
