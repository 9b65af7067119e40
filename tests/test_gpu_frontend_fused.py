"""Backward passes that no longer re-read a large tensor, against what they replace and against float64:
  * conv1's weight / bias gradient formed in the tile epilogue of the second convolution's input-gradient launch
    (eamd_conv2_bwd_x_conv1_bwd_w) against the stored input gradient + eamd_conv1_bwd_w;
  * the convolution's bias gradient as column sums of the weight-gradient GEMM's B operand;
  * the CTC gradient kernel run in backward with the upstream scalar read on the device (eamd_ctc_grad).
reference: transformer/subsampling.py:14-59,123-168 (Conv2dSubsampling, Conv2dSubsampling8), ctc.py:53-66."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from espnet_amd import ops as o
    o.set_precision("fp32")
    return o


def rel_err(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-30))


# ---------------------------------------------------------------------------------------------
# conv1 dw / db from the conv2 input-gradient kernel
# ---------------------------------------------------------------------------------------------
_front = {}


def front_case(ops, shape, Cc):
    """inputs on the device, the float64 autograd gradients of conv1's weight / bias, and the two-launch route's results;
    computed once per case and left unchanged"""
    key = (shape, Cc)
    if key in _front:
        return _front[key]
    from espnet_amd import functional as Fn
    B, T, F = shape
    g = torch.Generator().manual_seed(100 * T + Cc)
    x = torch.randn(B, T, F, generator=g)
    w1 = torch.randn(Cc, 1, 3, 3, generator=g) / 3.0
    b1 = torch.randn(Cc, generator=g) * 0.1
    w2 = torch.randn(Cc, Cc, 3, 3, generator=g) / (3.0 * Cc ** 0.5)
    b2 = torch.randn(Cc, generator=g) * 0.1
    H1, W1 = (T - 3) // 2 + 1, (F - 3) // 2 + 1
    H2, W2 = (H1 - 3) // 2 + 1, (W1 - 3) // 2 + 1
    dy2 = torch.randn(B, Cc, H2, W2, generator=g)
    # float64 reference: autograd of relu(conv2d(relu(conv2d(x)), stride 2)) for conv1's parameters
    w1r, b1r = w1.double().requires_grad_(), b1.double().requires_grad_()
    y1r = torch.relu(torch.nn.functional.conv2d(x.double()[:, None], w1r, b1r, stride=2))
    y2r = torch.relu(torch.nn.functional.conv2d(y1r, w2.double(), b2.double(), stride=2))
    (y2r * dy2.double()).sum().backward()
    xd = x.to(DEV)
    y1 = ops.conv1_fwd(xd, w1.to(DEV), b1.to(DEV), B, T, F, Cc, torch.float32).view(-1, Cc)
    y2, wd, Ho, Wo = Fn._conv3s2_fwd(y1, w2.to(DEV), b2.to(DEV), B, H1, W1, Cc, torch.float32)
    assert (Ho, Wo) == (H2, W2)
    dy = (dy2.permute(0, 2, 3, 1).reshape(-1, Cc).to(DEV) * (y2 > 0)).contiguous()
    dims = (B, H1, W1, Ho, Wo, Cc)

    def two_launch():
        dw2, db2 = torch.zeros(Cc, Cc, 3, 3, device=DEV), torch.zeros(Cc, device=DEV)
        dw1, db1 = torch.zeros(Cc, 1, 3, 3, device=DEV), torch.zeros(Cc, device=DEV)
        dy_in = Fn._conv3s2_bwd(dy, y1, wd, dw2, db2, *dims, torch.float32)
        ops.conv1_bwd_w(dy_in, xd, dw1, db1, B, T, F, Cc)
        return dw1, db1, dw2, db2
    _front[key] = dict(x=xd, y1=y1, wd=wd, dy=dy, dims=dims, dw_ref=w1r.grad, db_ref=b1r.grad, two=two_launch())
    return _front[key]


def fused(c, into=None):
    from espnet_amd import functional as Fn
    Cc = c["dims"][-1]
    dw2, db2 = torch.zeros(Cc, Cc, 3, 3, device=DEV), torch.zeros(Cc, device=DEV)
    dw1, db1 = into if into is not None else (torch.zeros(Cc, 1, 3, 3, device=DEV), torch.zeros(Cc, device=DEV))
    Fn._conv3s2_bwd_conv1w(c["dy"], c["y1"], c["wd"], dw2, db2, *c["dims"], c["x"], dw1, db1)
    return dw1, db1, dw2, db2


@pytest.mark.parametrize("Cc", [128, 256])
@pytest.mark.parametrize("shape", [(2, 41, 23), (3, 67, 27), (1, 40, 25)])
def test_fused_conv1_gradient_vs_float64(ops, shape, Cc):
    """error = |d|/|ref| against float64 autograd; yardstick = the two-launch route (_conv3s2_bwd, then ops.conv1_bwd_w) on the
    same inputs: the fused error may be at most twice its error, with the 2e-5 floor each of those two kernels is held to on
    its own (test_conv1_bwd_w_deterministic, test_conv2_input_gradient_classes_in_one_launch)"""
    c = front_case(ops, shape, Cc)
    dw_f, db_f, dw2_f, db2_f = fused(c)
    dw_t, db_t, dw2_t, db2_t = c["two"]
    for name, f, t, ref in (("dw", dw_f, dw_t, c["dw_ref"]), ("db", db_f, db_t, c["db_ref"])):
        ef, et = rel_err(f, ref), rel_err(t, ref)
        print(f"[parity] fused conv1 {name} {shape} C={Cc}: fused {ef:.3e} two-launch {et:.3e}")
        assert ef <= max(2.0 * et, 2e-5), (name, ef, et)
    # the second convolution's own gradients do not depend on the route (split-K atomics: to rounding)
    assert rel_err(dw2_f, dw2_t) <= 2e-6 and rel_err(db2_f, db2_t) <= 2e-6
    assert rel_err(db2_f, c["dy"].double().sum(0)) <= 1e-5


@pytest.mark.parametrize("shape,Cc", [((3, 67, 27), 128), ((2, 41, 23), 256)])
def test_fused_conv1_gradient_accumulates_and_repeats(ops, shape, Cc):
    c = front_case(ops, shape, Cc)
    dw_a, db_a, _, _ = fused(c)
    dw_b, db_b, _, _ = fused(c)
    assert torch.equal(dw_a, dw_b) and torch.equal(db_a, db_b)          # equal inputs: equal bits
    dw_c, db_c = dw_a.clone(), db_a.clone()
    fused(c, into=(dw_c, db_c))                                          # a second call into non-zero buffers doubles them
    assert rel_err(dw_c, 2 * c["dw_ref"]) <= max(2.0 * rel_err(c["two"][0], c["dw_ref"]), 2e-5)
    assert rel_err(db_c, 2 * c["db_ref"]) <= max(2.0 * rel_err(c["two"][1], c["db_ref"]), 2e-5)
    assert torch.equal(dw_c, dw_a + dw_a) and torch.equal(db_c, db_a + db_a)


# ---------------------------------------------------------------------------------------------
# module level
# ---------------------------------------------------------------------------------------------
def module_grads(mod, x, fuse):
    from espnet_amd import functional as Fn
    keep, Fn.FUSE_CONV1_WGRAD = Fn.FUSE_CONV1_WGRAD, fuse
    try:
        mod.zero_grad(set_to_none=True)
        y, _ = mod(x, None)
        (y * y).sum().backward()
        return [p.grad.clone() for p in mod.parameters()], y.detach().clone()
    finally:
        Fn.FUSE_CONV1_WGRAD = keep


@pytest.mark.parametrize("cls,T", [("Conv2dSubsampling", 41), ("Conv2dSubsampling8", 67)])
def test_subsampling_modules_with_and_without_the_fused_route(ops, cls, T):
    """forward + backward of the module with the flag on and off: every parameter gradient agrees within the bar of the
    kernel test (the stored-gradient route is the yardstick: twice its error is at most 4e-5, so 4e-5 between the two)"""
    from espnet_amd.nets import modules as M
    torch.manual_seed(3)
    mod = getattr(M, cls)(23, 128, 0.0).to(DEV)
    x = torch.randn(2, T, 23, device=DEV)
    g_on, y_on = module_grads(mod, x, True)
    g_off, y_off = module_grads(mod, x, False)
    assert torch.equal(y_on, y_off)
    for (name, _), a, b in zip(mod.named_parameters(), g_on, g_off):
        e = rel_err(a, b)
        print(f"[parity] {cls} {name}: fused vs stored route {e:.3e}")
        assert e <= 4e-5, (name, e)


def test_subsampling_forward_backward_in_a_graph(ops):
    """forward + backward captured in a graph: two replays give the eager gradients (to the rounding of the split-K atomics
    some of them pass through: 2e-6, the bar of the fp32 GEMM tests)"""
    from espnet_amd.nets import modules as M
    torch.manual_seed(4)
    mod = M.Conv2dSubsampling(23, 128, 0.0).to(DEV)
    x = torch.randn(2, 41, 23, device=DEV)
    eager, _ = module_grads(mod, x, True)
    names = [n for n, _ in mod.named_parameters()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        module_grads(mod, x, True)                   # warm-up on the capture stream
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        mod.zero_grad(set_to_none=True)
        with torch.cuda.graph(graph, stream=side):
            y, _ = mod(x, None)
            (y * y).sum().backward()
    torch.cuda.current_stream().wait_stream(side)
    held = [p.grad for p in mod.parameters()]
    for _ in range(2):
        for gbuf in held:
            gbuf.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for n, a, b in zip(names, held, eager):
            assert rel_err(a, b) <= 2e-6, (n, rel_err(a, b))


# ---------------------------------------------------------------------------------------------
# column sums of the B operand in the gathered weight-gradient GEMM
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splitk", [2, 7])
@pytest.mark.parametrize("Cc,tile", [(64, 64), (128, 128)])
def test_weight_gradient_gemm_sums_the_columns_of_b(ops, Cc, tile, splitk):
    """the conv2 weight-gradient product dwf = col^T dy with colsum: db against the float64 column sums of dy at 1e-5, dwf
    as without colsum (split-K atomics add in any order: 2e-6, the bar of the fp32 GEMM tests)"""
    from espnet_amd import functional as Fn
    B, Hi, Wi = 3, 21, 13
    Ho, Wo = (Hi - 3) // 2 + 1, (Wi - 3) // 2 + 1
    M = B * Ho * Wo
    assert M % 32 != 0
    g = torch.Generator().manual_seed(Cc + splitk)
    y_in = torch.randn(B * Hi * Wi, Cc, generator=g).to(DEV)
    dy = torch.randn(M, Cc, generator=g).to(DEV)
    gat = ops.make_gather(Cc, Fn._TAPS_FWD, Ho, Wo, Hi, Wi, 2, 2)

    def run(db):
        dwf = torch.zeros(9 * Cc, Cc, device=DEV)
        ops.gemm(y_in, dy, dwf, 9 * Cc, Cc, M, 9 * Cc, Cc, Cc, transA=1, transB=1, gather=gat, splitk=splitk, tile=tile, colsum=db)
        return dwf
    db = torch.zeros(Cc, device=DEV)
    with_sum, without = run(db), run(None)
    e = rel_err(db, dy.double().sum(0))
    print(f"[parity] B-side colsum C={Cc} tile={tile} splitk={splitk}: db {e:.3e} dwf {rel_err(with_sum, without):.3e}")
    assert e <= 1e-5
    assert rel_err(with_sum, without) <= 2e-6
    run(db)                                                    # accumulates
    assert rel_err(db, 2 * dy.double().sum(0)) <= 1e-5


# ---------------------------------------------------------------------------------------------
# CTC gradient in backward
# ---------------------------------------------------------------------------------------------
def ctc_case(time_major):
    B, T, V, L = 3, 17, 50, 5
    g = torch.Generator().manual_seed(17)
    acts = torch.randn(B, T, V, generator=g)
    ys = torch.tensor([[3, 7, 3, 9, 11], [5, 6, 7, -1, -1], [2, 4, 8, 16, 32]], dtype=torch.int64)
    il = torch.tensor([17, 12, 9], dtype=torch.int32)
    if time_major:
        acts = acts.transpose(0, 1).contiguous()
    return acts.to(DEV), ys.to(DEV), il.to(DEV), B, T, V, L


@pytest.mark.parametrize("time_major", [False, True])
def test_ctc_gradient_pass_with_device_scalar(ops, time_major):
    acts, ys, il, B, T, V, L = ctc_case(time_major)
    gs = torch.tensor(0.3, device=DEV)
    nll, grad = ops.ctc_loss(acts, ys, il, 0, -1, 1.0 / B, time_major=time_major)
    want = ops.scale_dev(grad, gs)
    nll2, none, ws = ops.ctc_loss(acts, ys, il, 0, -1, 1.0 / B, want_grad=False, time_major=time_major, keep_workspace=True)
    assert none is None and torch.equal(nll, nll2)
    got = ops.ctc_grad(acts, il, nll2, ws, L, 0, 1.0 / B, gscale=gs.view(1), time_major=time_major)
    assert torch.equal(got, want)
    assert torch.equal(ops.ctc_grad(acts, il, nll2, ws, L, 0, 1.0 / B, time_major=time_major), grad)      # no scalar
    gb = got if not time_major else got.transpose(0, 1)
    for b in range(B):
        assert float(gb[b, int(il[b]):].abs().max() if int(il[b]) < T else 0.0) == 0.0
        assert float(gb[b, :int(il[b])].abs().max()) > 0.0


@pytest.mark.parametrize("time_major", [False, True])
def test_ctc_loss_function_through_autograd(ops, time_major):
    from espnet_amd import functional as Fn
    acts, ys, il, B, T, V, L = ctc_case(time_major)
    nll, grad = ops.ctc_loss(acts, ys, il, 0, -1, 1.0 / B, time_major=time_major)
    want_loss = ops.reduce_sum(nll, 1.0 / B)
    a = acts.clone().requires_grad_()
    loss = Fn.CTCLossFn.apply(a, ys, il, 0, -1, time_major)
    (loss * 0.3).sum().backward()
    assert torch.equal(loss.detach().reshape(-1), want_loss.reshape(-1))
    assert torch.equal(a.grad, ops.scale_dev(grad, torch.tensor(0.3, device=DEV)))
