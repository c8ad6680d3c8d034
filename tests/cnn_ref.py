"""The crowd policy's convolution trunk restated in float64 with torch.nn.functional.conv2d on the CPU -- TEST INFRASTRUCTURE ONLY.

What emloco_cnn_trunk computes (include/emloco_predictor.h): the map columns normalised and clamped as RunningMeanStd does, viewed as
(rows, res, res, channels) channel last, permuted to NCHW, Conv2d(kernel 4, stride 2, padding 1) + ReLU per layer, flattened in
(channel, row, column) order."""
import numpy as np
import torch
import torch.nn.functional as F


def normalize(x, mean, var, eps, clip):
    x, mean, var = (np.asarray(a, np.float64) for a in (x, mean, var))
    return np.clip((x - mean) / np.sqrt(var + np.float64(np.float32(eps))), -clip, clip)


def trunk(maps, res, channels, weights, biases, mean=None, var=None, eps=1e-5, clip=5.0):
    """maps (rows, channels * res * res) raw (mean / var given) or already normalised (None) -> (features (rows, F * side^2) float64,
    [every layer's activations, float64])"""
    x = np.asarray(maps, np.float64)
    if mean is not None:
        x = normalize(x, mean, var, eps, clip)
    t = torch.from_numpy(x).reshape(x.shape[0], res, res, channels).permute(0, 3, 1, 2)
    acts = []
    for w, b in zip(weights, biases):
        t = torch.relu(F.conv2d(t, torch.from_numpy(np.asarray(w, np.float64)), torch.from_numpy(np.asarray(b, np.float64)), stride=2, padding=1))
        acts.append(t.numpy())
    return t.reshape(t.shape[0], -1).numpy(), acts
