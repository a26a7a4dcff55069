"""lc_train_transform_rows on the MI355X: the train transform written straight into conv1's bf16
patch rows for any even patch size at a padded row stride (ViT-L/14: patch 14, 588 data columns
in rows of 640), and what stands on it: TrainTransform / EvalTransform(layout="patches") for a
patch-14 model, the image tower taking those rows, and OnlineLoop with both transforms.

The rows are compared bit for bit with the two launches they replace (lc_train_transform layout 0
+ lc_patchify_pad), on the separable LDS kernel (small inputs; grids of g = 2, 4 and 16 patch rows
in bands of one patch row, and of several for large batches) and on the gather kernel (in both of
its normalisation forms), and against the oracle at the bound of
test_kernels_gpu.py::test_train_transform_vs_oracle (one bf16 step)."""
import pytest
import torch

from oracle import clip_oracle as o

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
QNAN = 0x7FC0  # bf16 quiet NaN: a byte the launch did not write stays visible
GUARD = 8
MEAN, STD = (0.5071, 0.4867, 0.4408), (0.2675, 0.2565, 0.2761)
PARAMS = [(0, 0, False), (8, 8, True), (3, 6, True)]


def batch(n, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, 3, H, W), generator=g).float() / 255  # ToTensor values


def nan_rows(rows, ldo, dev):
    """(whole buffer with GUARD rows on either side, the [rows, ldo] view handed to the launch)"""
    buf = torch.full((rows + 2 * GUARD, ldo), QNAN, device=dev, dtype=torch.int16).view(BF)
    return buf, buf[GUARD:GUARD + rows]


def guards_intact(buf):
    raw = buf.view(torch.int16)
    return bool((raw[:GUARD] == QNAN).all() and (raw[-GUARD:] == QNAN).all())


def two_launch_rows(tf, x, params, P, ldo):
    """What a patch-14 loop needed before: the f32 batch, then lc_patchify_pad."""
    from lcclip import ops
    img = tf(x, params=params, layout="nchw")
    g = tf.inp_size // P
    return ops.patchify_pad(img, P, torch.empty(x.shape[0] * g * g, ldo, device=x.device, dtype=BF))


@pytest.mark.parametrize("H,W", [(32, 32), (20, 36)])
@pytest.mark.parametrize("R", [28, 56, 224])
def test_rows_equal_transform_then_patchify_pad(dev, R, H, W):
    """LDS path, patch 14: every crop / flip / uint8-round-trip / stride combination."""
    from lcclip.transforms import TrainTransform
    x = batch(3, H, W, seed=R + H).to(dev)
    g = R // 14
    for autoaug in (True, False):
        tf = TrainTransform(MEAN, STD, inp_size=R, padding=4, autoaug=autoaug, patch=14)
        for params in PARAMS:
            for ldo in (640, 704):
                want = two_launch_rows(tf, x, params, 14, ldo)
                buf, out = nan_rows(3 * g * g, ldo, dev)
                got = tf(x, params=params, layout="patches", out=out)
                assert got.data_ptr() == out.data_ptr()
                assert torch.equal(got, want), (autoaug, params, ldo)
                assert guards_intact(buf)
        # the default buffer: conv1's width
        rows = tf(x, params=PARAMS[2], layout="patches")
        assert rows.shape == (3 * g * g, 640) and rows.dtype == BF
        assert torch.equal(rows, two_launch_rows(tf, x, PARAMS[2], 14, 640))


def test_rows_with_autoaugment_ops_in_front(dev):
    from lcclip.transforms import TrainTransform
    from test_autoaug_gpu import images
    x = images(3, 32, 32, seed=9).to(dev)
    tf = TrainTransform(MEAN, STD, patch=14)
    params = ([("Equalize", 0.0), ("Rotate", 15.0)], 3, 6, True)
    got = tf(x, params=params, layout="patches")
    assert torch.equal(got, two_launch_rows(tf, x, params, 14, 640))


@pytest.mark.parametrize("n,R", [(1100, 28), (600, 56), (342, 56)])
def test_rows_bands_of_several_patch_rows(dev, n, R):
    """The host splits an image's g patch rows into bands, about four workgroups per CU (256
    CUs): large batches get bands of more than one patch row. 1100 images at g = 2: one band of
    2; 600 at g = 4: two bands of 2; 342 at g = 4: three bands of 1, 1 and 2."""
    from lcclip.transforms import TrainTransform
    x = batch(n, 32, 32, seed=n).to(dev)
    tf = TrainTransform(MEAN, STD, inp_size=R, patch=14)
    for params in PARAMS[1:]:
        got = tf(x, params=params, layout="patches")
        assert torch.equal(got, two_launch_rows(tf, x, params, 14, 640)), params


def test_rows_gather_path(dev):
    """Inputs the layout-0 LDS kernel does not take (3 x 96 x 96 f32 > 64 KiB) go to the gather
    kernel, normalised as (v - mean) / std like train_transform_kernel."""
    from lcclip.transforms import TrainTransform
    x = batch(3, 96, 96, seed=5).to(dev)
    tf = TrainTransform(MEAN, STD, patch=14)
    for params in PARAMS:
        for ldo in (640, 704):
            buf, out = nan_rows(3 * 256, ldo, dev)
            got = tf(x, params=params, layout="patches", out=out)
            assert torch.equal(got, two_launch_rows(tf, x, params, 14, ldo)), (params, ldo)
            assert guards_intact(buf)


def test_rows_gather_path_fused_normalise(dev):
    """A band whose source rows do not fit LDS (one 224-pixel patch of a 64 x 64 image: all 64
    source rows at 224 columns, 172 KB) takes the gather kernel too, but layout 0 still runs its
    LDS kernel there, which normalises with one FMA: the gather kernel follows."""
    from lcclip.transforms import TrainTransform, train_transform_rows
    x = batch(2, 64, 64, seed=8).to(dev)
    tf = TrainTransform(MEAN, STD, patch=224)
    ldo = 3 * 224 * 224 + 64
    for params in PARAMS[1:]:
        want = two_launch_rows(tf, x, params, 224, ldo)
        buf, out = nan_rows(2, ldo, dev)
        train_transform_rows(x, out, MEAN, STD, 224, 224, 4, params[:2], params[2], True)
        assert torch.equal(out, want), params
        assert guards_intact(buf)


@pytest.mark.parametrize("H,W", [(32, 32), (96, 96)], ids=["lds", "gather"])
def test_every_byte_written(dev, H, W):
    from lcclip.transforms import TrainTransform
    x = batch(3, H, W, seed=11).to(dev)
    tf = TrainTransform(MEAN, STD, patch=14)
    for ldo in (640, 704):
        buf, out = nan_rows(3 * 256, ldo, dev)
        tf(x, params=(8, 8, True), layout="patches", out=out)
        assert not torch.isnan(out.float()).any()
        assert (out[:, 588:].view(torch.int16) == 0).all()
        assert out[:, :588].float().abs().max().item() > 0.5
        assert guards_intact(buf)


@pytest.mark.parametrize("H,W", [(32, 32), (64, 64), (96, 96)])
def test_patch16_through_the_rows_entry(dev, H, W):
    from lcclip.transforms import TrainTransform, train_transform_rows
    x = batch(3, H, W, seed=13).to(dev)
    tf = TrainTransform(MEAN, STD, patch=16)
    i, j, flip = 3, 6, True
    want = tf(x, params=(i, j, flip), layout="patches")
    assert want.shape == (3 * 196, 768)
    _, out = nan_rows(3 * 196, 768, dev)
    train_transform_rows(x, out, MEAN, STD, 224, 16, 4, (i, j), flip, True)
    assert torch.equal(out, want)
    buf, wide = nan_rows(3 * 196, 832, dev)
    assert tf(x, params=(i, j, flip), layout="patches", out=wide).data_ptr() == wide.data_ptr()
    assert torch.equal(wide[:, :768], want)
    assert (wide[:, 768:].view(torch.int16) == 0).all()
    assert guards_intact(buf)


@pytest.mark.parametrize("params", PARAMS)
def test_rows_vs_oracle(dev, params):
    """One bf16 step from patchify(oracle), the bound of test_train_transform_vs_oracle."""
    from lcclip.transforms import TrainTransform
    i, j, flip = params
    x = batch(3, 32, 32, seed=sum(params[:2]) + 1)
    tf = TrainTransform(MEAN, STD, patch=14)
    ref = o.patchify(o.train_transform(x, 224, 4, i, j, flip, tf.mean, tf.std, quantize=True), 14)
    assert ref.shape == (3 * 256, 588)
    got = tf(x.to(dev), params=params, layout="patches").float().cpu()
    d = (got[:, :588] - ref).abs()
    assert (d <= ref.abs() * 2 ** -7 + 1e-6).all(), d.max().item()
    assert (got[:, 588:] == 0).all()


@pytest.mark.parametrize("patch,ldo", [(14, 584), (14, 644), (7, 192)])
def test_refusals_launch_nothing(dev, patch, ldo):
    from lcclip.transforms import TrainTransform
    x = batch(2, 32, 32, seed=3).to(dev)
    g = 224 // patch
    buf, out = nan_rows(2 * g * g, ldo, dev)
    with pytest.raises(Exception, match="lc_train_transform_rows returned -1"):
        TrainTransform(MEAN, STD, patch=patch)(x, params=(0, 0, False), layout="patches", out=out)
    torch.cuda.synchronize()
    assert (buf.view(torch.int16) == QNAN).all()


# ------------------------------------------------------------------- the tower and the trainer
def small_wrapper(dev):
    from test_model_gpu import make_wrapper
    from test_vit_l14_gpu import SMALL
    sd = o.synthetic_state_dict(SMALL, "adapter", "both", seed=31)
    return SMALL, make_wrapper(sd, "adapter", "both", dev)


def test_tower_takes_the_rows(dev):
    """conv1's GEMM sees identical operands either way: features and one whole step agree."""
    from lcclip import OnlineTrainer
    from lcclip.transforms import TrainTransform, patch_row_width
    cfg, w = small_wrapper(dev)
    assert patch_row_width(cfg.vision_patch_size) == 640
    x = batch(4, 32, 32, seed=17).to(dev)
    tf = TrainTransform(MEAN, STD, patch=14)
    prm = (3, 6, True)
    rows, img = tf(x, params=prm, layout="patches"), tf(x, params=prm, layout="nchw")
    assert rows.shape == (4 * 256, 640)
    with torch.no_grad():
        assert torch.equal(w.encode_image(rows), w.encode_image(img))
    tok = o.synthetic_tokens(4, cfg.context_length, seed=33, vocab=cfg.vocab_size).to(dev)
    y = (torch.arange(4) % 4).to(dev)
    probs = []
    for inp in (rows, img):
        _, wi = small_wrapper(dev)
        _, p = OnlineTrainer(wi).step(inp, y, tok)
        probs.append(p.clone())
    torch.cuda.synchronize()
    assert torch.isfinite(probs[0]).all()
    assert torch.equal(probs[0], probs[1])


class NchwFeed:
    """The same transform, handed to the model as the f32 batch."""

    def __init__(self, tf):
        self.tf = tf

    def __call__(self, x, layout="patches"):
        assert layout == "patches"
        return self.tf(x, layout="nchw")


def run_loop(dev, feed):
    from lcclip import OnlineTrainer
    from lcclip.online import OnlineLoop
    from lcclip.stream import ClassBook, SiBlurryStream
    from lcclip.transforms import EvalTransform, TrainTransform
    cfg, w = small_wrapper(dev)
    imgs = batch(8, 8, 8, seed=4)
    labels = torch.tensor([0, 1, 0, 1, 2, 3, 3, 2])
    class_tokens = o.synthetic_tokens(4, 77, seed=12, vocab=cfg.vocab_size)
    stream = SiBlurryStream(labels.tolist(), 4, 2, m=0, n=100, rnd_seed=3)
    book = ClassBook([f"class{i}" for i in range(4)])
    tf = TrainTransform.for_dataset("cifar100", patch=14,
                                    generator=torch.Generator().manual_seed(6))
    ev = EvalTransform.for_dataset("cifar100", patch=14)
    losses = []
    loop = OnlineLoop(OnlineTrainer(w, lr=2e-3), stream, book, imgs, labels, imgs, labels,
                      lambda ns: class_tokens[torch.tensor([int(n[5:]) for n in ns])].to(dev),
                      transform=feed(tf), eval_transform=feed(ev), batch_size=4, online_iter=1,
                      on_step=lambda k, loss, acc: losses.append(loss))
    return loop.run(), losses


def test_online_loop_with_both_transforms(dev):
    res, losses = run_loop(dev, lambda tf: tf)
    assert res["steps"] == 2 and len(losses) == 2
    assert all(l == l and abs(l) != float("inf") for l in losses), losses
    acc = res["task_records"]["task_acc"]
    assert len(acc) == 2 and all(0.0 <= a <= 1.0 for a in acc)
    res2, losses2 = run_loop(dev, NchwFeed)
    assert res2["task_records"]["task_acc"] == acc
    assert res2["task_records"]["cls_acc"] == res["task_records"]["cls_acc"]


def test_eval_transform_is_the_plain_train_launch(dev):
    from lcclip.transforms import EvalTransform, TrainTransform
    x = batch(3, 8, 8, seed=2).to(dev)
    ev = EvalTransform(MEAN, STD, patch=14)
    tf = TrainTransform(MEAN, STD, padding=0, autoaug=False, patch=14)
    for layout in ("nchw", "patches"):
        assert torch.equal(ev(x, layout=layout), tf(x, params=(0, 0, False), layout=layout))
    assert ev(x, layout="patches").shape == (3 * 256, 640)
    ev16, tf16 = EvalTransform(MEAN, STD), TrainTransform(MEAN, STD, padding=0, autoaug=False)
    assert torch.equal(ev16(x, layout="patches"), tf16(x, params=(0, 0, False), layout="patches"))
