"""The backward of the crowd policy's convolution trunk in float64 (torch autograd over torch.nn.functional.conv2d on the CPU) -- TEST
INFRASTRUCTURE ONLY.

What emloco_cnn_trunk_backward computes (include/emloco_predictor.h): with L = sum(features * dout) over the trunk of tests/cnn_ref.py,
dL/dW and dL/db of every layer, summed over the rows.  `backward` also returns every layer's pre-activation, so that a test can hold the
inputs to a margin around the ReLU's corner, and checks its own forward against cnn_ref.trunk."""
import numpy as np
import torch
import torch.nn.functional as F

import cnn_ref


def backward(maps, res, channels, weights, biases, dout, mean=None, var=None, eps=1e-5, clip=5.0, dtype=torch.float64):
    """maps (rows, channels * res * res) raw (mean / var given) or normalised; dout (rows, features) ->
    ([(dW, db) per layer], [pre-activation per layer], features), numpy arrays of `dtype`"""
    x = np.asarray(maps, np.float64)
    if mean is not None:
        x = cnn_ref.normalize(x, mean, var, eps, clip)
    t = torch.from_numpy(x).to(dtype).reshape(x.shape[0], res, res, channels).permute(0, 3, 1, 2)
    ws = [torch.from_numpy(np.asarray(w, np.float64)).to(dtype).requires_grad_() for w in weights]
    bs = [torch.from_numpy(np.asarray(b, np.float64)).to(dtype).requires_grad_() for b in biases]
    pre = []
    for w, b in zip(ws, bs):
        z = F.conv2d(t, w, b, stride=2, padding=1)
        pre.append(z.detach().numpy())
        t = torch.relu(z)
    feat = t.reshape(t.shape[0], -1)
    if dtype == torch.float64:
        ref, _ = cnn_ref.trunk(x, res, channels, weights, biases)
        assert np.array_equal(ref, feat.detach().numpy())
    (feat * torch.from_numpy(np.asarray(dout, np.float64)).to(dtype)).sum().backward()
    return [(w.grad.numpy(), b.grad.numpy()) for w, b in zip(ws, bs)], pre, feat.detach().numpy()
