"""engine.py::_msg_vectors_pack without a GPU: the slices of the three layers that read the message channels (c0 and res_conv of the first
bottleneck block, the first Upsample group's nine-tap GEMM) and the rows appended to the message GEMM reassemble to the packed originals."""
import torch

from videoseal_amd.engine import ConvW, HipEngine


def test_sliced_and_appended_weights_reassemble_to_the_packed_originals():
    g = torch.Generator().manual_seed(3)
    nlat, hidden, co = 32, 64, 16
    n = nlat + hidden                                   # the bottleneck keeps its width: cout = bott
    c0 = ConvW(torch.randn(n, 9 * n, generator=g), torch.randn(n, generator=g), n, 3, 3, n)
    res = ConvW(torch.randn(n, n, generator=g), torch.randn(n, generator=g), n, 1, 1, n)
    gm = ConvW(torch.randn(9 * co, 2 * n, generator=g), None, 9 * co, 1, 1, 2 * n)          # K = [x (n) | latent skip | message skip]
    E = dict(bott=[dict(c0=c0, res=res, cout=n)], ups=[dict(gemm=gm)])
    v = HipEngine._msg_vectors_pack(E, nlat, hidden)
    msg = v["msg"]
    assert msg.N == msg.wt.shape[0] == 9 * n + n + 9 * co and msg.CinP == hidden and msg.wt.shape[1] == hidden
    assert v["off_res"] == 9 * n and v["off_up"] == 10 * n and v["off_res"] % 4 == 0 and v["off_up"] % 4 == 0 and msg.N % 4 == 0
    # c0: [N][9][lat | msg] <- latent conv + tap rows (tap, n) of the message GEMM
    taps = msg.wt[: 9 * n].view(9, n, hidden).permute(1, 0, 2)
    assert torch.equal(torch.cat([v["c0_lat"].wt.view(n, 9, nlat), taps], 2).reshape(n, 9 * n), c0.wt)
    assert v["c0_lat"].bias is c0.bias and (v["c0_lat"].N, v["c0_lat"].KH, v["c0_lat"].CinP) == (n, 3, nlat)
    # res_conv: [N][lat | msg], its bias rides in the message GEMM's bias (the per-frame bias2 = W_msg x latent + bias)
    assert torch.equal(torch.cat([v["res_lat"].wt, msg.wt[9 * n: 10 * n]], 1), res.wt)
    assert v["res_lat"].bias is None and torch.equal(msg.bias[9 * n: 10 * n], res.bias)
    assert not msg.bias[: 9 * n].any() and not msg.bias[10 * n:].any()
    # Upsample GEMM: [9 co][x | lat | msg]; the message-skip rows carry connect_scale = 2^-0.5 (the skip is scaled before the concat)
    assert torch.equal(v["up_xl"].wt, gm.wt[:, : n + nlat]) and v["up_xl"].CinP == n + nlat and v["up_xl"].bias is None
    assert torch.equal(msg.wt[10 * n:], gm.wt[:, n + nlat:] * (2 ** -0.5))
    assert all(t.is_contiguous() for t in (msg.wt, v["c0_lat"].wt, v["res_lat"].wt, v["up_xl"].wt))
