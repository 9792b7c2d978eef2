"""What tests/test_freeze_host.py and tests/test_freeze_gpu.py share: the model builder of tests/test_model_gpu.py (the same
configuration and procedural weights) and the freeze cases - the sets of parameters with requires_grad False that Train.py:115-121
(a `freeze` list of name fragments) and its commented block at :328-333 (everything under image_encoder) produce."""
import importlib

PKG = "small-object-detection-transformers_amd"
E = "image_encoder."
HEAD = [[2, 1, "Conv", [512, 1, 1]], [-1, 1, "nn.Upsample", [None, 2, "nearest"]], [[-1, 1], 1, "Concat", [1]],
        [-1, 3, "C3", [512, False]], [-1, 1, "Conv", [256, 1, 1]], [-1, 1, "nn.Upsample", [None, 2, "nearest"]],
        [[-1, 0], 1, "Concat", [1]], [-1, 3, "C3", [256, False]], [[10], 1, "Detect", ["nc", "anchors"]]]


def config(img, nc=8, sr=False):
    cfg = dict(nc=nc, depth_multiple=0.33, width_multiple=0.5, anchors=[[10, 13, 16, 30, 33, 23]],
               backbone=[[-1, 1, "ImageEncoderViT", [img, 6, 192, 4, 256, 4]]], head=[list(r) for r in HEAD])
    if sr:
        cfg.update(l1=4, l2=8, c1=128, c2=512)
    return cfg


def build(dev, img, nc=8, sr=False):
    """tests/test_model_gpu.py::build (sr: tests/test_model_sr_gpu.py::build): Model on `dev` with the oracle's procedural weights"""
    from oracle import ref_torch as R
    M = importlib.import_module(PKG + ".model")
    model = M.Model(config(img, nc, sr), input_mode="RGB+IR", ch_steam=3, ch=128, nc=nc, **(dict(sr=True, factor=2) if sr else {}))
    sd = R.procedural_state_dict(img, nc)
    if sr:
        S = importlib.import_module(PKG + ".sr")
        sd.update(R.procedural_from_shapes({"model_up." + k: v for k, v in S.sr_param_shapes(4, 128, 512).items()}))
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    assert all(("relative_position_index" in k or "attn_mask" in k) for k in missing), missing
    return model.to(dev), sd


STAGE1_PREFIX = (E + "channel_embed_", E + "chan_block.", E + "patch_embed.", E + "pos_embed", E + "stage1.")

# case -> predicate(name, parameter) -> frozen
CASES = {
    "nothing": lambda n, p: False,
    "encoder": lambda n, p: n.startswith(E),                        # Train.py:328-333
    "through_stage1": lambda n, p: n.startswith(STAGE1_PREFIX),     # front end + patch / pos embed + stage 1
    "stage2.1": lambda n, p: n.startswith(E + "stage2.1."),
    "detect": lambda n, p: n.startswith("detect."),                 # the whole head (model.detect holds every head row)
    "1d": lambda n, p: p.dim() == 1,
    "everything": lambda n, p: True,
    "model_up": lambda n, p: n.startswith("model_up."),             # Model(sr=True) only
}
ROWS = [c for c in CASES if c != "model_up"]


def apply(model, case):
    """set requires_grad of every parameter from the case; returns the set of frozen names"""
    frozen = set()
    for n, p in model.named_parameters():
        f = bool(CASES[case](n, p))
        p.requires_grad_(not f)
        if f:
            frozen.add(n)
    return frozen
