"""The identity behind the pooled-resolution stem tail (elem.cuh: stem_tail_kernel, stem_moments_kernel, stem_combine_kernel):

    dW0[c, t] = sum_n ( a_nc * T1_n[c, t]  +  b_nc * sum_t' w[c, t'] * R_n[t', t]  +  c_nc * S_n[t] )

checked in float64 against torch autograd on a tiny stem (conv 7x7 / 2 / 3 without bias over three identical channels,
training-mode BatchNorm per stream, ReLU, max pool 3 / 2 / 1).  The coefficients are those of the BN-backward operand
A = a * ((dy - q1) - (x - mean) * k) of the stem weight gradient: a = gamma * invstd, b = -a * k, c = a * (k * mean - q1) with
q1 = s1 / HW, k = invstd * s2 / HW, and s1 / s2 summed at POOLED resolution (the ReLU mask of the argmax element is X1 > 0)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

EPS = 1e-5
C = 6          # output channels of the tiny stem; the last one is pooled to zero everywhere
TOL = 1e-10


def _formula(imgs, W0, gamma, beta, gup):
    """numpy restatement: imgs [n][H][W], W0 [C][3][7][7], gup [n][C][Hq][Wq] -> dW0 [C][3][7][7], dbeta [C], dgamma [C]"""
    n_streams, H, W = imgs.shape
    Hs, Ws = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    Hq, Wq = (Hs - 1) // 2 + 1, (Ws - 1) // 2 + 1
    w = W0.sum(axis=1).reshape(C, 49)
    dw = np.zeros((C, 49))
    dbeta = np.zeros(C)
    dgamma = np.zeros(C)
    for n in range(n_streams):
        pad = np.zeros((H + 6 + 1, W + 6 + 1))          # I_n, zero outside [0, H) x [0, W)  (index = coordinate + 3)
        pad[3:3 + H, 3:3 + W] = imgs[n]
        # patches[p, t] = I[2p + t - 3]
        patches = np.zeros((Hs, Ws, 49))
        for ty in range(7):
            for tx in range(7):
                patches[:, :, ty * 7 + tx] = pad[ty:ty + 2 * Hs:2, tx:tx + 2 * Ws:2]
        x = patches @ w.T                                # [Hs][Ws][C]
        mean = x.mean(axis=(0, 1))
        invstd = 1.0 / np.sqrt(x.var(axis=(0, 1)) + EPS)
        xhat = (x - mean) * invstd
        y = np.maximum(gamma * xhat + beta, 0.0)
        R = np.einsum('yxs,yxt->st', patches, patches)   # image moments: the image only
        S = patches.sum(axis=(0, 1))
        T1 = np.zeros((C, 49))
        s1 = np.zeros(C)
        s2 = np.zeros(C)
        for qy in range(Hq):
            for qx in range(Wq):
                for c in range(C):
                    best, pos = -np.inf, None
                    for k in range(9):                   # the kernel's scan: first strict maximum of the window inside the plane
                        yy, xx = 2 * qy - 1 + k // 3, 2 * qx - 1 + k % 3
                        if 0 <= yy < Hs and 0 <= xx < Ws and y[yy, xx, c] > best:
                            best, pos = y[yy, xx, c], (yy, xx)
                    gm = gup[n, c, qy, qx] if best > 0.0 else 0.0      # X1[q, c] > 0: the argmax element passed the ReLU
                    s1[c] += gm
                    s2[c] += gm * xhat[pos[0], pos[1], c]
                    T1[c] += gm * patches[pos[0], pos[1]]
        HW = Hs * Ws
        a = gamma * invstd
        q1, kk = s1 / HW, invstd * s2 / HW
        b = -a * kk
        cc = a * (kk * mean - q1)
        dw += a[:, None] * T1 + b[:, None] * (w @ R) + cc[:, None] * S[None, :]
        dbeta += s1
        dgamma += s2
    return np.repeat(dw.reshape(C, 1, 7, 7), 3, axis=1), dbeta, dgamma


@pytest.mark.parametrize("n_streams", [1, 2])
@pytest.mark.parametrize("shape", [(40, 40), (44, 36)])
def test_stem_tail_identity(n_streams, shape):
    g = torch.Generator().manual_seed(1000 * n_streams + shape[0])
    H, W = shape
    # non-zero up to the border: the windows cut by the edge and the zero padding of R and S count
    imgs = torch.randn(n_streams, H, W, generator=g, dtype=torch.float64) + 0.5
    W0 = (0.2 * torch.randn(C, 3, 7, 7, generator=g, dtype=torch.float64)).requires_grad_()
    gamma = (0.5 + torch.rand(C, generator=g, dtype=torch.float64)).requires_grad_()
    beta_v = 0.3 * torch.randn(C, generator=g, dtype=torch.float64)
    beta_v[C - 1] = -50.0                               # |xhat| <= sqrt(HW) < 50 / gamma: this channel is zero after the ReLU
    beta = beta_v.requires_grad_()
    Hq, Wq = ((H - 1) // 2 + 1 - 1) // 2 + 1, ((W - 1) // 2 + 1 - 1) // 2 + 1
    gup = torch.randn(n_streams, C, Hq, Wq, generator=g, dtype=torch.float64)
    pooled_all = []
    for n in range(n_streams):                          # one BatchNorm batch per stream
        x3 = imgs[n].expand(1, 3, H, W)
        st = F.conv2d(x3, W0, stride=2, padding=3)
        yb = F.relu(F.batch_norm(st, None, None, gamma, beta, True, 0.0, EPS))
        pooled = F.max_pool2d(yb, 3, 2, 1)
        assert pooled.shape[2:] == (Hq, Wq)
        pooled_all.append(pooled.detach())
        (pooled * gup[n:n + 1]).sum().backward()
    assert float(torch.stack(pooled_all)[:, :, C - 1].abs().max()) == 0.0
    assert float(torch.stack(pooled_all)[:, :, 0].abs().max()) > 0.0

    dw, dbeta, dgamma = _formula(imgs.numpy(), W0.detach().numpy(), gamma.detach().numpy(), beta.detach().numpy(), gup.numpy())
    for name, got, ref in (("dW0", dw, W0.grad.numpy()), ("dbeta", dbeta, beta.grad.numpy()), ("dgamma", dgamma, gamma.grad.numpy())):
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print("%s: relative error %.3g" % (name, err))
        assert err <= TOL, (name, err)
    assert np.abs(W0.grad.numpy()[C - 1]).max() <= TOL * np.abs(W0.grad.numpy()).max()
