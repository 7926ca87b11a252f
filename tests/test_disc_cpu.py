"""The discriminator's host side without a GPU: the fixtures' own conditions (tests/golden/make_golden_disc.py), the state-dict contract of
`videoseal_amd.discriminator.NLayerDiscriminator` against the reference's as recorded in the fixture, its initialisation, what the HIP path refuses,
and that the training steps construct without touching a device."""
import numpy as np
import pytest
import torch

from tests import _disc_util as U
from tests._util import load_golden


@pytest.fixture(scope="module")
def ops():
    return load_golden("disc_ops")


@pytest.fixture(scope="module")
def steps():
    return load_golden("disc_step")


@pytest.mark.parametrize("case", U.CASES, ids=U.case_name)
def test_fixture_inputs_are_recreated_and_meet_the_kink_conditions(ops, case):
    name = U.case_name(case)
    m = ops["meta"]["cases"][name]
    assert tuple(m["case"]) == case
    sd, sdh = U.state_dict(case[0], case[1]), U.state_dict(case[0], case[1], hinge=True, hinge_seed=m["hinge_seed"])
    cs = U.checksum(U.frames(case, m["seed"], 0), U.frames(case, m["seed"], 1), U.dlogits(case), *sd.values(), *sdh.values())
    assert np.allclose(cs, ops[name + "/checksum"], rtol=1e-12, atol=0), "the seeded inputs differ from the ones the fixture was made with"
    # LeakyReLU kink: no pre-activation of the float64 run within the threshold of zero
    assert m["kink_threshold"] == 1e-6 and m["min_abs_lrelu_input"] >= m["kink_threshold"]
    # hinge kink: both ReLU masks are exercised and no logit sits on a kink
    assert m["hinge_share_real_above_1"] >= 0.1 and m["hinge_share_fake_below_m1"] >= 0.1 and m["hinge_gap"] >= 1e-4
    for k in m["keys"]:
        e, stats = ops[f"{name}/{k}.e"], ops[f"{name}/{k}.stats"]
        assert (e >= 0).all() and e[0] < 1e-3 and e[1] < 1e-3, (k, e, stats)


def test_step_fixture_is_complete(steps):
    cases = steps["meta"]["cases"]
    assert len(cases) == 16
    for name, m in cases.items():
        assert set(m["log"]) == ({"total_loss", "loss_percep", "loss_disc", "loss_decode", "scale_percep", "scale_disc", "scale_decode"}
                                 if m["optimizer_idx"] == 0 else {"disc_loss", "disc_factor", "logits_real", "logits_fake"}), name
        assert all(0 <= v < 1e-3 * max(1.0, abs(m["log"][k])) for k, v in m["log_e"].items()), (name, m["log_e"])
        below = m["global_step"] < m["disc_start"]
        if m["optimizer_idx"] == 0:
            assert (m["log"]["scale_disc"] == 0) == below
            assert all(k.startswith("disc.") for k in m["no_grad_params"]) and len(m["no_grad_params"]) == 12
        else:
            assert m["log"]["disc_factor"] == (0.0 if below else 1.0)
            assert m["no_grad_params"] and not any(k.startswith("disc.") for k in m["no_grad_params"])


@pytest.mark.parametrize("case", U.CASES, ids=U.case_name)
def test_state_dict_has_the_reference_names_shapes_and_dtypes(ops, case):
    from videoseal_amd.discriminator import NLayerDiscriminator
    ref = ops["meta"]["cases"][U.case_name(case)]["state_dict"]
    d = NLayerDiscriminator(input_nc=case[1], ndf=U.NDF, n_layers=case[0])
    got = [[k, list(v.shape), str(v.dtype)] for k, v in d.state_dict().items()]
    assert got == ref
    # a reference-format state dict (every name of the reference, nothing else) loads strictly
    sd = U.state_dict(case[0], case[1])
    assert sorted(sd) == sorted(k for k, _, _ in ref)
    d.load_state_dict(sd, strict=True)
    assert torch.equal(d.main[0].weight, sd["main.0.weight"])
    with pytest.raises(RuntimeError):
        d.load_state_dict({k: v for k, v in sd.items() if k != "rgb2yuv.M"}, strict=True)


def test_reference_constructor_defaults_and_initialisation():
    import inspect
    from videoseal_amd.discriminator import NLayerDiscriminator
    sig = inspect.signature(NLayerDiscriminator.__init__)
    assert [(k, p.default) for k, p in list(sig.parameters.items())[1:]] == [("input_nc", 3), ("ndf", 32), ("n_layers", 3), ("use_actnorm", False)]
    torch.manual_seed(7)
    d = NLayerDiscriminator(input_nc=3, ndf=32, n_layers=3)
    for m in d.main:
        if isinstance(m, torch.nn.Conv2d) and m.weight.numel() >= 4096:         # weights_init: N(0, 0.02)
            assert abs(float(m.weight.detach().std()) - 0.02) <= 0.002 and abs(float(m.weight.detach().mean())) < 0.002
        if isinstance(m, torch.nn.GroupNorm):                                   # everything else: torch's default
            assert m.num_groups == 4 and m.eps == 1e-5 and bool((m.weight == 1).all()) and bool((m.bias == 0).all())
    w = torch.cat([m.weight.flatten() for m in d.main if isinstance(m, torch.nn.Conv2d)])
    assert abs(float(w.detach().std()) - 0.02) <= 0.002


def test_what_the_hip_path_does_not_build_raises_with_the_reason():
    from videoseal_amd import discriminator as D
    from videoseal_amd.training import DiscriminatorStep, GeneratorStep
    with pytest.raises(NotImplementedError, match="use_actnorm"):
        D.NLayerDiscriminator(use_actnorm=True)
    with pytest.raises(NotImplementedError, match="vanilla"):
        DiscriminatorStep(D.NLayerDiscriminator(n_layers=2), disc_loss="vanilla")
    with pytest.raises(NotImplementedError, match="vanilla"):
        GeneratorStep(None, disc_weight=0.1, disc_loss="vanilla")
    with pytest.raises(NotImplementedError, match="cond"):
        D.NLayerDiscriminator(n_layers=2)(torch.zeros(1, 3, 32, 32), cond=torch.zeros(1, 1, 32, 32))
    with pytest.raises(NotImplementedError, match="cond"):
        DiscriminatorStep(D.NLayerDiscriminator(n_layers=2)).step(torch.zeros(1, 3, 32, 32), torch.zeros(1, 3, 32, 32), cond=torch.zeros(1, 1, 32, 32))
    with pytest.raises(NotImplementedError, match="UNetDiscriminatorSN"):
        D.UNetDiscriminatorSN(3)


def test_no_cpu_fallback():
    from videoseal_amd import native as N
    from videoseal_amd.discriminator import NLayerDiscriminator
    with pytest.raises(N.NativeError):
        NLayerDiscriminator(n_layers=2)(torch.zeros(1, 3, 32, 32))


def test_steps_construct_without_a_model_or_a_device():
    from videoseal_amd.training import GeneratorStep
    s = GeneratorStep(None, percep_loss="mse")
    assert s.disc_weight == 0.0 and s.discriminator is None
    assert GeneratorStep(None, percep_loss="ssim").percep_loss == "ssim"
    s = GeneratorStep(None, disc_weight=0.1)
    assert s.disc_weight == 0.1 and s.disc_start == 0 and s.disc_num_layers == 2 and s.disc_in_channels == 3
    assert s.discriminator is None, "the discriminator is built on first use, never in __init__"
    d = s.disc()
    assert d is s.disc() and d.n_layers == 2 and d.input_nc == 3 and all(p.device.type == "cpu" for p in d.parameters())
