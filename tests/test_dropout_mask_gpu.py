"""Every kernel that regenerates the dropout mask, against the host port of dropout_cases.py: the mask never comes from a
kernel's own output.  Each entry point runs with p > 0 and with p = 0 on the same inputs:

  forward    y_p == y_0 * scale_port BIT FOR BIT: the masked output is one more float32 multiply in the same kernel
             instance (o *= drop_scale(...) behind a run-time branch), and the unmasked run's mean / rstd come back unchanged;
  the rest   yn, mean, rstd against float64 on the explicitly masked row, the backward (g_z, g_gamma, g_beta; g_x, g_w, g_b
             for the layer kernels) against float64 through LayerNorm * mask_port -- by the bounds the p = 0 case of the
             same entry carries: per element against torch's float32 (rowwise_cases.check_layernorm_fwd / _bwd, as
             test_rowwise_conditioning_gpu.test_layernorm) for ops.act_layernorm, the largest error over the largest
             entry <= autograd_cases.PRODUCT against float64 autograd (as test_autograd_surface_gpu.py) for the layers.

Which call site draws the mask (csrc/lkg_rowwise.hip, lkg_gemm_tall.hip, lkg_layer.hip):

  act_ln_fwd_narrow_kernel<8 | 16 | 32>   forward, d % 4 == 0, d <= 128: d = 20, 32 | 48, 64 | 100, 128
  act_ln_fwd_kernel<4, 1..4>              forward, d % 4 == 0, d > 128: d = 132, 256 | 260, 512 | 516, 768 | 772, 1024
  act_ln_fwd_kernel<1, 1..4>              forward, scalar: d = 7, 63 | 65 | 129 | 193, 255, and d = 64, 256 from a misaligned base
  act_ln_bwd_narrow_kernel                backward, 16-byte, d <= 128, n >= 4096 (n = 4099: a ragged last group), y kept, dense
                                          output; with the row flags of g_yn ("yn on some rows")
  act_ln_bwd_kernel<W, CPL>               every other backward: n = 37, d > 128, scalar; with the row flags; through a row list
                                          (listed rows only, -1 padding, a zero table as g_z: the mask is the ABSOLUTE row's)
  act_ln_bwd_kernel, y not kept           the last layer's recompute of y on the rows g_yn reaches (want_y = False): its own site
  the tall GEMM's act + LayerNorm epilogue   ops.linear_act_layernorm: n_out = 7, 32, 128, 200, 256; m = 16384 (the fewest rows
                                          fused_layer_ok accepts) and 16389; its backward recomputes z and runs act_ln_bwd_*
                                          (dense, and on the listed rows of a row-sparse gradient)
  lkg_narrow_layer_bwd_f32                ops.narrow_layer, n = 4099 and 8200: dense gradients, and g_yn on some rows"""
import functools
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import autograd_cases as G
import dropout_cases as D
import op_audit as A
import rowwise_cases as C

pytestmark = pytest.mark.gpu

PS = (0.1, 0.5, 0.999)
SEEDS = (0, (1 << 32) - 1, (0x5DEECE66 << 32) | 0x0000000D)        # 0, one below 2^32, one with the high word set
NARROW16 = (20, 32, 48, 64, 100, 128)
GENERAL16 = (132, 256, 260, 512, 516, 768, 772, 1024)
SCALAR = (7, 63, 65, 129, 193, 255)
MISALIGNED = (64, 256)


@pytest.fixture(scope="module")
def ops(gpu_device):
    import __graft_entry__ as ge
    ge.build()
    from literalkg_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def N(ops):
    from literalkg_amd import _native
    return _native


@functools.lru_cache(maxsize=4)
def port_draws(seed, n, d):
    return D.draws(seed, np.arange(n), np.arange(d))


def port_scale(seed, n, d, p):
    """float32 [n, d] on the host: the port's scale of rows 0 .. n - 1"""
    return np.where(port_draws(seed, n, d) >= np.uint32(D.threshold(p)), D.inv_keep(p), np.float32(0)).astype(np.float32)


def host(t):
    return t.detach().cpu().numpy()


def leaf(t):
    return t.detach().clone().requires_grad_()


def same_bits(what, a, b):
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{what}: not the bits of the p = 0 run"


def kept_share_is_plausible(sc, p):
    """the port's own mask on this shape (a constant-true or constant-false scale would make every check below vacuous)"""
    D.check_count("kept share of the port's mask", int((sc != 0).sum()), sc.size, D.keep_prob(p), 1e-9)


# =============================================================================================== ops.act_layernorm
def act_ln(ops, case, p, seed, want_y=True):
    z, gamma, beta = leaf(case.z), leaf(case.gamma), leaf(case.beta)
    y, yn = ops.act_layernorm(z, gamma, beta, drop_p=p, seed=seed, want_y=want_y)
    saved = yn.grad_fn.saved_tensors
    return NS(z=z, gamma=gamma, beta=beta, y=y, yn=yn, mean=saved[3], rstd=saved[4])


def grads(run, outs, ups):
    gz, gg, gb = torch.autograd.grad(outs, (run.z, run.gamma, run.beta), ups)
    return dict(gz=gz, g_gamma=gg, g_beta=gb)


def with_upstream(case, gy, gyn):
    c = NS(**vars(case))
    c.gy, c.gyn = gy, gyn
    return c


def listed_rows(n, device, gen):
    """some 1/5 of the rows (the first, the last and every special row of draw_layernorm among them), with a duplicate"""
    pick = torch.rand(n, device=device, generator=gen) < 0.2
    pick[:6] = True
    pick[n - 1] = True
    return pick


def backward_through_row_list(ops, N, case, fwd, p, seed, pick, lines, what):
    """lkg_act_layernorm_bwd_f32 with a row list (sparse_out): the listed rows only, y NOT given (recomputed, mask and all),
    g_z a table that is zero elsewhere.  The list is shuffled and padded with -1."""
    dev, n, d = case.z.device, case.n, case.d
    ids = torch.nonzero(pick).flatten()
    ids = ids[torch.randperm(ids.numel(), device=dev, generator=torch.Generator(device=dev).manual_seed(n + d))]
    ids = torch.cat([ids[:3], torch.full((2,), -1, device=dev, dtype=torch.int64), ids[3:]]).contiguous()
    z, gy, gyn = ops._f32_rows(case.z), ops._f32_rows(case.gy), ops._f32_rows(case.gyn)
    nan = float("nan")
    gy_l = torch.where(pick[:, None], gy, torch.full_like(gy, nan))          # rows outside the list are not even read
    gyn_l = torch.where(pick[:, None], gyn, torch.full_like(gyn, nan))
    gz = torch.zeros(n, d, device=dev)
    gg, gb = torch.zeros(d, device=dev), torch.zeros(d, device=dev)
    N.call("lkg_act_layernorm_bwd_f32", n, d, N.ptr(z), ops._ld(z), case.slope, N.ptr(case.gamma), N.ptr(case.beta), None, 0,
           N.ptr(fwd.mean), N.ptr(fwd.rstd), N.ptr(gy_l), ops._ld(gy_l), N.ptr(gyn_l), ops._ld(gyn_l), case.norm_eps, N.ptr(gz), d,
           N.ptr(gg), N.ptr(gb), float(p), int(seed), None, None, 1, N.ptr(ids), ids.numel(), ops._stream())
    torch.cuda.synchronize()
    assert float(gz[~pick].abs().max()) == 0.0, f"{what}: wrote a row outside the list"
    zero = lambda t: torch.where(pick[:, None], t, torch.zeros_like(t))
    c = with_upstream(case, zero(gy), zero(gyn))
    c.what = what
    C.check_layernorm_bwd(lines, c, fwd.mean, fwd.rstd, fwd.y.detach(), dict(gz=gz, g_gamma=gg, g_beta=gb))


def act_layernorm_case(ops, N, device, n, d, offset):
    lines = []
    base = C.draw_layernorm(device, n, d, offset)
    gen = C.gen_for(device, 97 * d + n)
    pick = listed_rows(n, device, gen)
    r0 = act_ln(ops, base, 0.0, 0)
    for i, p in enumerate(PS):
        for j, seed in enumerate(SEEDS):
            what = f"n {n} d {d}{' offset' if offset else ''} p {p} seed {seed:#x}"
            sc = port_scale(seed, n, d, p)
            kept_share_is_plausible(sc, p) if n * d > 2000 else None
            r = act_ln(ops, base, p, seed)
            D.check_forward_bits(f"{what}: y", host(r.y), host(r0.y), sc)
            same_bits(f"{what}: mean", r.mean, r0.mean)
            same_bits(f"{what}: rstd", r.rstd, r0.rstd)
            if i != j:          # (the remaining checks on one seed per p)
                continue
            case = NS(**vars(base))
            case.drop, case.what = torch.from_numpy(sc).to(device), what
            C.check_layernorm_fwd(lines, case, dict(mean=r.mean, rstd=r.rstd, y=r.y.detach(), yn=r.yn.detach()))
            # ---- dense: g_y and g_yn everywhere
            C.check_layernorm_bwd(lines, case, r.mean, r.rstd, r.y.detach(), grads(r, (r.y, r.yn), (case.gy, case.gyn)))
            # ---- y not kept (the last layer): the backward recomputes the masked y of every row g_yn reaches
            r1 = act_ln(ops, base, p, seed, want_y=False)
            assert r1.y is None
            same_bits(f"{what}: yn without y", r1.yn.detach(), r.yn.detach())
            c1 = with_upstream(case, None, case.gyn)
            c1.what = what + " y not kept"
            C.check_layernorm_bwd(lines, c1, r.mean, r.rstd, r.y.detach(), grads(r1, (r1.yn,), (case.gyn,)), use_gy=False)
            # ---- g_yn on some rows only (row flags; too few rows to compact): with and without a dense g_y
            gyn_some = torch.where(pick[:, None], case.gyn, torch.zeros_like(case.gyn))
            for use_gy in (False, True):
                r2 = act_ln(ops, base, p, seed)
                tagged = ops.tag_rows(gyn_some.clone(), ops.RowSet(pick.to(torch.uint8), [torch.nonzero(pick).flatten()]))
                c2 = with_upstream(case, case.gy, gyn_some)
                c2.what = what + f" yn on some rows{', dense y' if use_gy else ''}"
                got = grads(r2, (r2.y, r2.yn) if use_gy else (r2.yn,), (case.gy, tagged) if use_gy else (tagged,))
                C.check_layernorm_bwd(lines, c2, r.mean, r.rstd, r.y.detach(), got, use_gy=use_gy)
            # ---- through a row list
            backward_through_row_list(ops, N, case, r, p, seed, pick, lines, what + " row list")
    return lines


@pytest.mark.parametrize("d,offset", [(d, False) for d in NARROW16 + GENERAL16 + SCALAR] + [(d, True) for d in MISALIGNED],
                         ids=lambda v: str(v))
def test_act_layernorm_draws_the_ports_mask(ops, N, gpu_device, d, offset):
    lines = []
    for n in (37, 4099):
        lines += act_layernorm_case(ops, N, gpu_device, n, d, offset)
    print(C.report(lines, 12))


# =============================================================================================== the layer kernels
def layer_inputs(device, n, ks, d, seed):
    """The draws of autograd_cases' layer entries, with x, w and bias rounded to multiples of 1/8, 1/16 and 1/16: every
    product and partial sum of z = x w^T + bias is then exact in each engine (fp16 hi parts hold such operands whole, float32
    adds multiples of 2^-7 below 2^17 without rounding), so the kernels' z IS the float64 z.  Otherwise some of the 10^5 ..
    10^6 LeakyReLU inputs of a case lie within a product's rounding of zero, the two take different slopes there, and the
    gradients differ by a finite step that says nothing about the mask (test_gpu_fuzz.py draws such cases again)."""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s, std=1.0: (torch.randn(*s, generator=gen) * std).to(device)
    grid = lambda t, q: torch.round(t * q) / q
    t = {f"x{i}": grid(rn(n, k, std=0.7), 8) for i, k in enumerate(ks)}
    t.update({f"w{i}": grid(rn(d, k, std=0.2), 16) for i, k in enumerate(ks)})
    t.update(bias=grid(rn(d, std=0.1), 16), gamma=1 + 0.1 * rn(d), beta=0.1 * rn(d))
    return t, rn(n, d), rn(n, d)


def layer_reference(t, n_terms, drop, outs, ups):
    """float64 autograd through Linear -> LeakyReLU -> LayerNorm -> * mask_port -> normalised copy: {slot: gradient}"""
    lv = {k: v.detach().double().requires_grad_() for k, v in t.items()}
    z = sum(lv[f"x{i}"] @ lv[f"w{i}"].t() for i in range(n_terms)) + lv["bias"]
    r = A.layernorm_fwd_eval(z, lv["gamma"], lv["beta"], G.LN_CFG["slope"], G.LN_CFG["eps"], G.LN_CFG["norm_eps"], torch.float64,
                             drop=drop)
    # (the normalised copy once more, differentiable on a row the mask emptied: sqrt has no derivative at 0, and at
    # p = 0.999 most rows are empty -- there yn = y / norm_eps, as in the kernels and in _ln_upstream)
    n2 = (r["y"] * r["y"]).sum(1, keepdim=True)
    big = n2 > G.LN_CFG["norm_eps"] ** 2
    r["yn"] = torch.where(big, r["y"] / torch.sqrt(torch.where(big, n2, torch.ones_like(n2))), r["y"] / G.LN_CFG["norm_eps"])
    torch.autograd.backward([r[o] for o in outs], [u.double() for u in ups])
    return r, {k: v.grad for k, v in lv.items()}


def check_layer_grads(what, got, want):
    for k, w in want.items():
        bad = G.judge64(G.PRODUCT, got[k], w)
        assert bad is None, f"{what}: gradient of {k}: {bad}"


def check_layer_forward(what, run, run0, sc, ref):
    D.check_forward_bits(f"{what}: y", host(run["y"]), host(run0["y"]), sc)
    same_bits(f"{what}: mean", run["mean"], run0["mean"])
    same_bits(f"{what}: rstd", run["rstd"], run0["rstd"])
    for k in ("y", "yn", "mean", "rstd"):
        bad = G.judge64(G.PRODUCT, run[k], ref[k])
        assert bad is None, f"{what}: {k}: {bad}"
    # the normalised copy per element, on the kernel's own masked y
    yp = run["y"].detach()
    want = yp.double() / torch.sqrt((yp.double() ** 2).sum(1, keepdim=True)).clamp_min(G.LN_CFG["norm_eps"])
    ref32 = yp / torch.sqrt((yp * yp).sum(1, keepdim=True)).clamp_min(G.LN_CFG["norm_eps"])
    C.check_reduction([], f"{what}: yn of the masked y", run["yn"].detach(), want, want.abs(), ref32)


def run_fused_layer(ops, t, ks, p, seed):
    lv = {k: leaf(v) for k, v in t.items()}
    xs, ws = [lv[f"x{i}"] for i in range(len(ks))], [lv[f"w{i}"] for i in range(len(ks))]
    y, yn = ops.linear_act_layernorm(xs, ws, lv["bias"], lv["gamma"], lv["beta"], drop_p=p, seed=seed)
    saved = y.grad_fn.saved_tensors
    return dict(lv=lv, y=y, yn=yn, mean=saved[2 * len(ks) + 2], rstd=saved[2 * len(ks) + 3])


@pytest.mark.parametrize("m", [16384, 16389])
@pytest.mark.parametrize("d,ks", [(7, (40,)), (32, (300,)), (128, (64, 64)), (200, (32, 8)), (256, (64,))], ids=lambda v: str(v))
def test_tall_epilogue_draws_the_ports_mask(ops, gpu_device, m, d, ks):
    assert ops.fused_layer_ok(m, d, ks) and not ops.fused_layer_ok(16383, d, ks)
    t, gy, gyn = layer_inputs(gpu_device, m, ks, d, m + d)
    r0 = run_fused_layer(ops, t, ks, 0.0, 0)
    # a row-sparse gradient of both outputs: 600 listed rows (with duplicates), worth compacting at 16384 rows
    gen = torch.Generator().manual_seed(d)
    ids = torch.cat([torch.tensor([0, m - 1, m - 1]), torch.randint(0, m, (597,), generator=gen)]).to(gpu_device)
    flags = torch.zeros(m, dtype=torch.uint8, device=gpu_device)
    flags[ids] = 1
    on = flags.bool()[:, None]
    gy_s, gyn_s = torch.where(on, gy, torch.zeros_like(gy)), torch.where(on, gyn, torch.zeros_like(gyn))
    for p, seed in zip(PS, SEEDS):
        what = f"m {m} ks {ks} -> {d} p {p} seed {seed:#x}"
        sc = port_scale(seed, m, d, p)
        kept_share_is_plausible(sc, p)
        drop = torch.from_numpy(sc).to(gpu_device)
        r = run_fused_layer(ops, t, ks, p, seed)
        ref, want = layer_reference(t, len(ks), drop, ("y", "yn"), (gy, gyn))
        check_layer_forward(what, r, r0, sc, ref)
        torch.autograd.backward([r["y"], r["yn"]], [gy, gyn])
        check_layer_grads(what + " dense", {k: v.grad for k, v in r["lv"].items()}, want)
        # on the listed rows: z recomputed there, the row-wise backward through its row list (absolute rows in the mask)
        r = run_fused_layer(ops, t, ks, p, seed)
        rows = ops.RowSet(flags, [ids])
        assert ops.rows_worth_compacting(rows, m)
        torch.autograd.backward([r["y"], r["yn"]], [ops.tag_rows(gy_s.clone(), rows), ops.tag_rows(gyn_s.clone(), rows)])
        _, want = layer_reference(t, len(ks), drop, ("y", "yn"), (gy_s, gyn_s))
        check_layer_grads(what + " listed rows", {k: v.grad for k, v in r["lv"].items()}, want)
        assert float(r["lv"]["x0"].grad[~flags.bool()].abs().max()) == 0.0
    ops._RowScratch._tables.clear()


def run_narrow_layer(ops, t, p, seed):
    lv = {k: leaf(v) for k, v in t.items()}
    assert ops.narrow_layer_ok(lv["x0"], lv["w0"])
    y, yn = ops.narrow_layer(lv["x0"], lv["w0"], lv["bias"], lv["gamma"], lv["beta"], drop_p=p, seed=seed)
    saved = y.grad_fn.saved_tensors
    return dict(lv=lv, y=y, yn=yn, mean=saved[5], rstd=saved[6])


@pytest.mark.parametrize("n", [4099, 8200])
def test_narrow_layer_draws_the_ports_mask(ops, gpu_device, n):
    t, gy, gyn = layer_inputs(gpu_device, n, (32,), 32, n)
    r0 = run_narrow_layer(ops, t, 0.0, 0)
    some = (torch.rand(n, generator=torch.Generator().manual_seed(n)) < 0.6).to(gpu_device)     # as test_gpu_parity's narrow-layer test
    some[n - 1] = True
    gyn_s = torch.where(some[:, None], gyn, torch.zeros_like(gyn))
    for p, seed in zip(PS, SEEDS):
        what = f"narrow layer n {n} p {p} seed {seed:#x}"
        sc = port_scale(seed, n, 32, p)
        kept_share_is_plausible(sc, p)
        drop = torch.from_numpy(sc).to(gpu_device)
        for tag, outs, ups in (("dense", ("y", "yn"), (gy, gyn)), ("y only", ("y",), (gy,)), ("yn on some rows", ("yn",), (gyn_s,)),
                               ("yn on some rows, flagged", ("yn",), (gyn_s,))):
            if p > 0.9 and outs == ("yn",):
                # at p = 0.999 and 32 columns nearly every row keeps no element or one, and the gradient of a row's normalised
                # copy with one element is exactly zero: "of the largest entry" has nothing to stand on without g_y
                continue
            r = run_narrow_layer(ops, t, p, seed)
            ref, want = layer_reference(t, 1, drop, outs, ups)
            if tag == "dense":
                check_layer_forward(what, r, r0, sc, ref)
            if "flagged" in tag:
                ups = (ops.tag_rows(gyn_s.clone(), ops.RowSet(some.to(torch.uint8), [torch.nonzero(some).flatten()])),)
            with G.launches() as seen:
                torch.autograd.backward([r[o] for o in outs], list(ups))
            assert "lkg_narrow_layer_bwd_f32" in seen, (what, tag, seen)        # the one-launch backward, not the unfused pair
            check_layer_grads(f"{what} {tag}", {k: v.grad for k, v in r["lv"].items()}, want)


# =============================================================================================== layer independence
def test_two_layers_of_one_forward_draw_their_own_seeds(ops, gpu_device, monkeypatch):
    """ops.new_seed hands every layer of a forward its own seed (from torch's CPU generator: the same after the same
    torch.manual_seed), and each layer's mask is the port's for ITS seed."""
    seeds = []
    real = ops.new_seed

    def recording():
        seeds.append(real())
        return seeds[-1]

    monkeypatch.setattr(ops, "new_seed", recording)
    n, p, widths = 4099, 0.1, (64, 32, 32)
    t, _, _ = layer_inputs(gpu_device, n, (48,), 64, 5)
    w2, w3 = ((torch.randn(32, k, generator=torch.Generator().manual_seed(k)) * 0.2).to(gpu_device) for k in (64, 32))
    ln = lambda d: (torch.ones(d, device=gpu_device), torch.zeros(d, device=gpu_device))

    def forward(p_):
        y1, _ = ops.act_layernorm(ops.linear(t["x0"], t["w0"], t["bias"]), t["gamma"], t["beta"], drop_p=p_)
        y2, _ = ops.act_layernorm(ops.linear(y1, w2), *ln(32), drop_p=p_)
        assert ops.narrow_layer_ok(y2, w3)
        y3, _ = ops.narrow_layer(y2, w3, None, *ln(32), drop_p=p_)
        return y1, y2, y3

    torch.manual_seed(7)
    got = forward(p)
    assert len(seeds) == 3 and all(0 <= s < 1 << 63 for s in seeds)
    first = list(seeds)
    rows, cols = np.arange(n), [np.arange(w) for w in widths]
    # each layer against its own unmasked run on the SAME input (the masked output of the layer below)
    ins = (ops.linear(t["x0"], t["w0"], t["bias"]), ops.linear(got[0], w2), None)
    y0 = [ops.act_layernorm(ins[0], t["gamma"], t["beta"])[0], ops.act_layernorm(ins[1], *ln(32))[0],
          ops.narrow_layer(got[1], w3, None, *ln(32))[0]]
    for k in range(3):
        D.check_forward_bits(f"layer {k}", host(got[k]), host(y0[k]), D.scale(first[k], rows, cols[k], p))
    D.check_layer_seeds("three layers", first, [None] * 3, rows, cols, p)
    assert len(seeds) == 3                    # (no seed is drawn when p = 0)
    torch.manual_seed(7)
    again = forward(p)
    assert seeds[3:] == first and all(torch.equal(a, b) for a, b in zip(got, again))
    more = forward(p)
    assert len(set(seeds[:3] + seeds[6:])) == 6 and not torch.equal(more[0], got[0])
