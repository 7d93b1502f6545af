"""What the training path derives from the weights (fragment packs, fingerprints, CrossEmbed tables, the lagged mode's events and pinned
buffers) lives in train_ops' two weak side tables, and the inference engine belongs to ONE U-Net: parameters, modules, copies and pickles
carry none of it."""
import copy
import gc
import io

import pytest
import torch
import torch.nn.functional as F

from minimagen_amd import conv_route, train_ops
from minimagen_amd.Imagen import Imagen
from minimagen_amd.Unet import Unet
from oracle import restated as R
from tests._backend import setup
from tests.test_training import BASE


def tiny_imagen(unet):
    return Imagen((unet,), text_encoder_name="t5_small", image_sizes=(16,), timesteps=50, cond_drop_prob=0.).train()


def saved_size(module) -> int:
    buf = io.BytesIO()
    torch.save(module, buf)
    return buf.getbuffer().nbytes


def step(im, imgs, emb, mask, seed):
    """one identically seeded forward + backward -> (loss, gradients)"""
    for p in im.parameters():
        p.grad = None
    torch.manual_seed(seed)
    loss = im(imgs, text_embeds=emb, text_masks=mask)
    loss.backward()
    return loss.detach(), [p.grad for p in im.unets[0].parameters()]


def test_nothing_is_left_on_parameters_or_modules_and_copies_train_identically():
    setup("emu")
    torch.manual_seed(31)
    unet = Unet(**BASE)
    im = tiny_imagen(unet)
    imgs = torch.rand(2, 3, 16, 16)
    emb, mask = R.synthetic_text(2, length=9, seed=4)
    before = saved_size(unet)
    train_ops.FORCE = True
    try:
        loss, grads = step(im, imgs, emb, mask, 100)
        assert torch.isfinite(loss) and all(g is not None for g in grads)
        assert train_ops.step_state(unet) is not None and train_ops.weight_state(unet.final_conv.weight).fwd is not None      # the device path ran
        carriers = list(unet.parameters()) + list(unet.buffers()) + list(unet.modules())
        assert [(type(o).__name__, k) for o in carriers for k in vars(o) if k.startswith("_mi_")] == []
        after = saved_size(unet)
        print(f"torch.save(unet): {before} bytes before the step, {after} after")
        assert after == before
        twin = copy.deepcopy(unet)
        assert train_ops.step_state(twin) is None and all(train_ops.weight_state(p) is None for p in twin.parameters())
        a = step(im, imgs, emb, mask, 101)
        b = step(tiny_imagen(twin), imgs, emb, mask, 101)
    finally:
        train_ops.FORCE = False
    assert torch.equal(a[0], b[0])
    assert len(a[1]) == len(b[1]) and all(torch.equal(ga, gb) for ga, gb in zip(a[1], b[1]))


def test_the_side_tables_do_not_leak():
    """no table value holds a strong reference to its key or to a parameter: the entries die with the module and both tables are empty again.
    The tables are process-wide and other test modules keep trained modules alive in cached cases (functools.lru_cache), so "empty" is counted
    from what is alive before this test's module exists, after a collection: zero in a process of its own."""
    setup("emu")
    gc.collect()
    others = (len(train_ops._WEIGHTS), len(train_ops._STEPS))
    conv = torch.nn.Conv2d(8, 8, 3)
    train_ops.begin_step(conv)
    train_ops._packs(conv.weight)
    assert train_ops.step_state(conv) is not None and train_ops.weight_state(conv.weight).fwd is not None
    assert (len(train_ops._WEIGHTS), len(train_ops._STEPS)) == (others[0] + 1, others[1] + 1)
    del conv
    gc.collect()
    assert (len(train_ops._WEIGHTS), len(train_ops._STEPS)) == others


def test_a_deep_copy_of_a_unet_does_not_share_its_engine():
    """the engine owns workspaces and raw graph handles: a copy starts without one and builds its own, from the same weights, to the same bits"""
    setup("emu")
    torch.manual_seed(32)
    unet = Unet(**BASE).eval()
    x, tm = torch.randn(1, 3, 16, 16), torch.tensor([7])
    emb, mask = R.synthetic_text(1, length=9, seed=4)
    out = unet(x, tm, text_embeds=emb, text_mask=mask)
    assert unet._engine is not None
    twin = copy.deepcopy(unet)
    assert twin._engine is None and unet._engine is not None
    assert torch.equal(twin(x, tm, text_embeds=emb, text_mask=mask), out)
    assert twin._engine is not None and twin._engine is not unet._engine


# tile code of train_ops._conv3x3's row-paired launches before it took them from conv_route: rows Cin, columns Cout, both over CHANNELS
CHANNELS = (8, 16, 32, 64, 128)
TILE_CODES = {
    (8, 8): ((7, 7, 7, 7, 7), (7, 7, 7, 7, 7), (7, 7, 7, 7, 7), (7, 7, 7, 7, 7), (7, 7, 7, 7, 7)),
    (16, 16): ((7, 7, 7, 7, 7), (7, 7, 7, 7, 7), (7, 7, 7, 7, 7), (7, 7, 7, 7, 7), (7, 7, 7, 7, 7)),
    (32, 32): ((7, 7, 7, 7, 7), (7, 7, 7, 7, 7), (7, 7, 7, 7, 7), (7, 7, 7, 7, 7), (7, 7, 7, 7, 7)),
    (64, 64): ((7, 6, 7, 7, 7), (7, 6, 7, 7, 7), (7, 6, 7, 7, 7), (7, 6, 7, 7, 7), (7, 7, 7, 7, 7)),
    (128, 128): ((6, 6, 7, 7, 7), (6, 6, 7, 7, 7), (6, 6, 7, 7, 7), (6, 6, 7, 7, 7), (7, 7, 7, 7, 7)),
    (64, 256): ((6, 6, 7, 7, 7), (6, 6, 7, 7, 7), (6, 6, 7, 7, 7), (6, 6, 7, 7, 7), (7, 7, 7, 7, 7)),
}


def test_training_conv_tile_codes_are_the_ones_from_before_conv_route():
    for (H, W), table in TILE_CODES.items():
        for cin, row in zip(CHANNELS, table):
            for cout, code in zip(CHANNELS, row):
                family, got = conv_route.rp_code(cin, cout, H, W)
                assert got == code, (cin, cout, H, W, got, code)
                assert (family == conv_route.WIDE) == (not (cin <= 64 and cout <= 32)), (cin, cout)       # the wide regime's extra launch and buffers
        assert conv_route.direct_code(H, W) == (0 if (W >= 64 and H * W > 64 * 64) else 2)


@pytest.mark.gpu
def test_a_conv_that_trained_on_the_device_copies_and_pickles():
    """the lagged mode's events and pinned buffers are not reachable from the module: deepcopy and torch.save work, and the copy packs for itself"""
    dev = setup("gpu")
    assert train_ops.LAGGED
    torch.manual_seed(21)
    conv = torch.nn.Conv2d(8, 8, 3, padding=1).to(dev)
    x = torch.randn(2, 8, 16, 16, device=dev)
    for _ in range(2):
        train_ops.begin_step(conv)
    assert train_ops.step_state(conv).k == 2
    twin = copy.deepcopy(conv)
    torch.save(conv, io.BytesIO())
    assert train_ops.step_state(twin) is None and train_ops.weight_state(twin.weight) is None
    train_ops.begin_step(twin)
    y = train_ops.conv3x3_forward(twin, x)
    ref = F.conv2d(x.double(), conv.weight.detach().double(), conv.bias.detach().double(), padding=1)
    assert (y.double() - ref).abs().max() < 2e-6 * float(ref.abs().max())
