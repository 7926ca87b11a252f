"""Region-wise watermarks without a GPU: the torch definition (videoseal_amd/regions.py) against the reference's own blend on the CPU oracle,
label maps from masks, the integer label-sampling rule, every refusal with its exception type, and the discipline of the new public header
include/videoseal_regions.h (exported, bound, named in the GPU test, nothing of it declared in videoseal_hip.h)."""
import dataclasses
import os
import re

import pytest
import torch

from oracle import videoseal_ref as O
from oracle.inputs import synthetic_frames, synthetic_msgs
from oracle.weights import make_state_dict, tiny_spec
from tests._model import cfg_of
from videoseal_amd import native as N
from videoseal_amd import regions as RG
from videoseal_amd import rgbpack, yuv
from videoseal_amd.capi import CModel
from videoseal_amd.model import build_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _labels(F_, H, W, R, seed):
    """blocks, single pixels, a value above R and plenty of background"""
    g = torch.Generator().manual_seed(seed)
    lab = torch.zeros(F_, H, W, dtype=torch.uint8)
    lab[:, : H // 2, : W // 3] = 1
    lab[:, H // 3:, W // 2:] = 2 if R >= 2 else 1
    lab[:, 1::7, 2::5] = torch.randint(0, R + 2, lab[:, 1::7, 2::5].shape, generator=g, dtype=torch.uint8)      # R + 1: above R -> background
    return lab


# ---------------------------------------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("is_video", [False, True], ids=["image", "video"])
def test_the_definition_is_the_references_blend_per_region_bit_for_bit(is_video):
    spec = tiny_spec()
    sd = make_state_dict(spec, seed=3)
    F_, H, W = 4, 40, 56
    imgs = synthetic_frames(F_, H, W, seed=7)
    msgs = synthetic_msgs(2, spec.nbits, seed=8)
    labels = _labels(F_, H, W, 2, 9)
    if is_video:
        embed = lambda x, m: O.embed_video(sd, spec, x, m, chunk_size=2, step_size=2)["imgs_w"]                      # noqa: E731
    else:
        embed = lambda x, m: O.embed_image(sd, spec, x, m.repeat(len(x), 1))["imgs_w"]                                # noqa: E731
    per_region = [embed(imgs, msgs[r:r + 1]) for r in range(2)]
    assert not torch.equal(per_region[0], per_region[1]) and not torch.equal(per_region[0], imgs)
    want = RG.blend_reference(imgs, per_region, labels)             # x <- w_r * m_r + x * (1 - m_r), once per region
    got = RG.embed_regions(embed, imgs, labels, msgs)
    assert torch.equal(got, want)
    bg = (RG.clean_labels(labels, 2) == 0)[:, None].expand_as(imgs)
    assert bg.any() and torch.equal(got[bg], imgs[bg])
    for r in (1, 2):
        sel = (labels == r)[:, None].expand_as(imgs)
        assert sel.any() and torch.equal(got[sel], per_region[r - 1][sel])
    # one message per frame and region ([F, R, k]) is the image mode's other form
    if not is_video:
        m3 = msgs[None].repeat(F_, 1, 1)
        assert torch.equal(RG.embed_regions(lambda x, m: O.embed_image(sd, spec, x, m)["imgs_w"], imgs, labels, m3), want)


def test_compose_on_uint8_frames_copies_bytes():
    g = torch.Generator().manual_seed(1)
    x = torch.randint(0, 256, (2, 9, 11, 3), generator=g, dtype=torch.uint8)
    w = [torch.randint(0, 256, x.shape, generator=g, dtype=torch.uint8) for _ in range(3)]
    lab = torch.randint(0, 5, (2, 9, 11), generator=g, dtype=torch.uint8)
    out = RG.compose(x, w, lab)
    for f in range(2):
        for y in range(9):
            for xx in range(11):
                r = int(lab[f, y, xx])
                assert torch.equal(out[f, y, xx], x[f, y, xx] if r == 0 or r > 3 else w[r - 1][f, y, xx])


def test_labels_from_masks_highest_region_wins():
    m = torch.zeros(2, 3, 4, 5)
    m[:, 0, :, :3] = 1.0
    m[:, 1, 1:3, 2:] = 0.25            # non-zero selects
    m[0, 2, 2, 2] = -1.0
    lab = RG.labels_from_masks(m)
    assert lab.dtype == torch.uint8 and lab.shape == (2, 4, 5)
    want = torch.zeros(2, 4, 5, dtype=torch.uint8)
    want[:, :, :3] = 1
    want[:, 1:3, 2:] = 2
    want[0, 2, 2] = 3
    assert torch.equal(lab, want)
    assert torch.equal(RG.labels_from_masks(m.bool()), want)
    with pytest.raises(ValueError):
        RG.labels_from_masks(torch.zeros(1, 9, 4, 4))
    with pytest.raises(ValueError):
        RG.labels_from_masks(torch.zeros(4, 4))


@pytest.mark.parametrize("H,S", [(16, 16), (37, 16), (9, 16), (770, 256)])
def test_label_sampling_rule_against_a_literal_loop(H, S):
    got = RG.label_index(S, H).tolist()
    want = [((2 * i + 1) * H) // (2 * S) for i in range(S)]
    assert got == want and all(0 <= v < H for v in got) and got == sorted(got)
    if H == S:
        assert got == list(range(S))
    lab = (torch.arange(H * 3, dtype=torch.int64).view(1, H, 3) % 251).to(torch.uint8)
    at = RG.labels_at_map(lab, S, 3)
    for i in range(S):
        assert torch.equal(at[0, i], lab[0, want[i]])


def test_vote_and_decide_follow_the_references_selection():
    """bit_accuracy_inference (evals/metrics.py:208-256) restated with a mask per region"""
    g = torch.Generator().manual_seed(5)
    preds = torch.randn(2, 1 + 6, 8, 8, generator=g)
    lab = torch.randint(0, 3, (2, 8, 8), generator=g, dtype=torch.uint8)
    lab[1][lab[1] == 2] = 0                     # region 2 is empty in frame 1
    for method in RG.DECODE_METHODS:
        out = RG.decode_regions(preds, lab, 2, method=method)
        for f in range(2):
            for r in (1, 2):
                mask = (lab[f] == r)[None].expand(6, 8, 8)
                p = preds[f, 1:]
                vals = ((p > 0.0) if method == "hard" else p).masked_select(mask).view(6, -1)
                if vals.shape[1] == 0:
                    assert torch.isnan(out["score"][f, r - 1]).all() and not out["msgs"][f, r - 1].any() and int(out["count"][f, r - 1]) == 0
                    continue
                mean = vals.mean(dim=-1, dtype=float)
                assert torch.allclose(out["score"][f, r - 1], mean, rtol=1e-12, atol=1e-12)
                assert torch.equal(out["msgs"][f, r - 1], mean > 0.5) and int(out["count"][f, r - 1]) == vals.shape[1]
    clip = RG.decode_regions(preds, lab, 2, method="hard", per="clip")
    v, n, s = RG.vote_regions(preds[:, 1:], lab, 2)
    assert clip["score"].shape == (1, 2, 6) and torch.equal(clip["score"][0], v.sum(0).double() / n.sum(0).double()[:, None])


def test_label_boxes_definition():
    lab = torch.zeros(2, 6, 7, dtype=torch.uint8)
    lab[0, 1:3, 2:6] = 1
    lab[0, 5, 0] = 2
    lab[1, 0, 6] = 1
    b = RG.label_boxes(lab, 3)
    assert b[0].tolist() == [[1, 2, 3, 6], [5, 0, 6, 1], [0, 0, 0, 0]] and b[1].tolist() == [[0, 6, 1, 7], [0, 0, 0, 0], [0, 0, 0, 0]]


# ---------------------------------------------------------------------------------------------------------------- refusals
@pytest.fixture(scope="module")
def model():
    return build_model(cfg_of(tiny_spec())).eval()


def test_refusals_tell_the_reason(model):
    k = model.embedder.cfg.nbits
    imgs = torch.rand(2, 3, 8, 8)
    lab = torch.zeros(2, 8, 8, dtype=torch.uint8)
    msgs = torch.zeros(2, k)
    # clips in other formats and lists
    planes = (torch.zeros(2, 8, 8, dtype=torch.uint8), torch.zeros(2, 4, 8, dtype=torch.uint8))
    with pytest.raises(NotImplementedError, match="YUV and packed-RGB"):
        model.embed_regions(yuv.Clip(planes, "nv12"), lab, msgs)
    with pytest.raises(NotImplementedError, match="YUV and packed-RGB"):
        model.embed_regions(rgbpack.Clip(torch.zeros(2, 8, 8, 4, dtype=torch.uint8), "rgba"), lab, msgs)
    with pytest.raises(NotImplementedError, match="lists of images or clips"):
        model.embed_regions([imgs[0], imgs[1]], lab, msgs)
    with pytest.raises(NotImplementedError, match="lists of images or clips"):
        model.decode_regions([imgs], lab)
    with pytest.raises(NotImplementedError, match="lists of images or clips"):
        model.detect_regions((imgs,), lab, 2)
    # autograd
    with pytest.raises(NotImplementedError, match="autograd"):
        model.embed_regions(imgs.clone().requires_grad_(), lab, msgs)
    with pytest.raises(NotImplementedError, match="autograd"):
        model.embed_regions(imgs, lab, msgs.clone().requires_grad_())
    with pytest.raises(NotImplementedError, match="autograd"):
        model.decode_regions(imgs.clone().requires_grad_(), lab)
    # a target PSNR per region, the model-level C-ABI
    with pytest.raises(TypeError, match="labels"):              # embed_psnr keeps its signature: it has no label map to take
        model.embed_psnr(imgs, 40.0, labels=lab)
    for name in ("embed_regions", "decode_regions", "detect_regions"):
        with pytest.raises(NotImplementedError, match="vs_model_"):
            getattr(CModel, name)(None, imgs, lab)
    # arguments
    with pytest.raises(TypeError, match="uint8"):
        model.embed_regions(imgs, lab.float(), msgs)
    with pytest.raises(ValueError, match="do not match"):
        model.embed_regions(imgs, lab[:, :4], msgs)
    with pytest.raises(ValueError, match="between 1 and 8"):
        model.embed_regions(imgs, lab, torch.zeros(9, k))
    with pytest.raises(ValueError, match="between 1 and 8"):
        model.detect_regions(imgs, lab, 0)
    with pytest.raises(ValueError, match="one message per region"):
        model.embed_regions(imgs, lab, torch.zeros(2, 2, k), is_video=True)
    with pytest.raises(ValueError, match="rows of regions"):
        model.embed_regions(imgs, lab, torch.zeros(3, 2, k), is_video=False)
    with pytest.raises(ValueError, match="RGB24"):
        model.embed_regions(torch.zeros(2, 8, 8, 4, dtype=torch.uint8), lab, msgs)
    # decoding: the method, and which detector each call is for
    with pytest.raises(NotImplementedError, match="fractional"):
        model.decode_regions(imgs, lab, method="soft")
    with pytest.raises(ValueError, match="unknown method"):
        model.decode_regions(imgs, lab, method="majority")
    with pytest.raises(ValueError, match="per must be"):
        model.decode_regions(imgs, lab, per="chunk")
    assert not model.pixelwise
    with pytest.raises(NotImplementedError, match="detect_regions"):
        model.decode_regions(imgs, lab)
    pw = build_model(dataclasses.replace(cfg_of(tiny_spec(dims=[16, 32, 64, 128])), head_stages=[4, 4, 2], head_pixelwise=True)).eval()
    with pytest.raises(NotImplementedError, match="decode_regions"):
        pw.detect_regions(imgs, lab, 2)


# ---------------------------------------------------------------------------------------------------------------- the header
def _declared(name):
    text = open(os.path.join(ROOT, "include", name)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return re.findall(r"(?m)^\s*(?:const\s+)?[A-Za-z_]\w*(?:\s*\*)?\s+\*?(vs_\w+)\s*\(", text)


def test_every_declaration_of_the_regions_header_is_exported_bound_and_tested():
    decl = _declared("videoseal_regions.h")
    assert sorted(decl) == sorted(N.REGION_EXPORTS) and len(set(decl)) == len(decl) == 4
    main = set(_declared("videoseal_hip.h"))
    assert len(main) > 150 and not main & set(decl) and not set(N.EXPORTS) & set(decl)
    header = open(os.path.join(ROOT, "include", "videoseal_regions.h")).read()
    assert re.search(r"#define\s+VS_REGIONS_MAX\s+8\b", header) and N.REGIONS_MAX == RG.REGIONS_MAX == 8
    assert "tests/_ledger.py" in header.split("#ifndef")[0]                # the opening comment says why the header stands alone
    lib = N.lib()
    gpu_test = open(os.path.join(ROOT, "tests", "test_gpu_regions.py")).read()
    for sym in decl:
        assert hasattr(lib, sym), f"{sym} is declared but not exported"
        assert getattr(lib, sym).argtypes, f"{sym} has no ctypes signature in native.py"
        assert re.search(r"\b" + sym + r"\b", gpu_test), f"{sym} is not named in tests/test_gpu_regions.py"
    assert lib.vs_pixel_vote_regions_partial_doubles.restype is not None and lib.vs_pixel_vote_regions_partial_doubles(3, 5, 4097, 4) > 0
    # argument checks happen on the host before any launch: refused without a GPU
    d = N.TailDesc()
    assert lib.vs_embed_tail_regions(None, None, 1, None) == -1 and lib.vs_embed_tail_regions(d, None, 1, None) == -1
    assert lib.vs_label_boxes(None, 1, 1, 1, 1, None, None) == -1
    assert lib.vs_pixel_vote_regions(None, 0, None, 1, 1, 1, 1, 1, 1, 1, 0.0, None, None, None, None, None) == -1
    for bad in (0, 9, -1):
        assert lib.vs_pixel_vote_regions_partial_doubles(1, 1, 1, bad) == -1
