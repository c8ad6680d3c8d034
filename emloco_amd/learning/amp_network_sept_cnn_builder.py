"""AMPSeptCNNBuilder -- the PACER policy / critic / discriminator network that reads the crowd sensor's rows, its convolution
trunk on the fused gfx950 kernel `emloco_cnn_trunk` (csrc/cnn_kernels.hip) and, where asked for, its backward
`emloco_cnn_trunk_backward` (csrc/cnn_backward_kernels.hip).

Mirror of /root/reference/pacer/pacer/learning/amp_network_sept_cnn_builder.py:17-164 (AMPSeptCNNBuilder.Network) over
amp_network_builder.py:16-124 and network_builder.py:125-148 / 165-277 for `amp_humanoid_smpl_cnn_task.yaml` (network `amp_sept_cnn`).
The reference class derives from AMPBuilder.Network and has no `_task_mlp`; here it derives from this repository's
AMPSeptBuilder.Network (which already restates AMPBuilder.Network: actor / critic MLPs, heads, sigma, discriminator) and replaces the
task MLP with the CNN parts, so the parameters, their names and their order are the reference's and its checkpoints load with
`strict=True`: `sigma`, `actor_mlp.*`, `critic_mlp.*`, `value`, `mu`, `_disc_mlp.*`, `_disc_logits`, `_task_actor_cnn.{0,2,4}`,
`_cnn_mlp.{0,2}` (only when the map is not 32 x 32), `_task_critic_cnn.{0,2,4}` (when `separate`).

`eval_task(task_obs)`: the first `detail['traj']` columns are the path; the rest is the map, viewed (B, res, res, C) channel last
(C = 1 for `heightmap`, 3 for `heightmap_velocity`, res = sqrt(F / C)), through `_task_actor_cnn` (Conv2d(kernel 4, stride 2,
padding 1) + ReLU per entry of `task_cnn.convs`), flattened (channel, row, column); where res != 32 through `_cnn_mlp` (Linear ->
512, ReLU, Linear -> 256, ReLU: widths fixed, the discriminator's activation); the result is cat([features, path]).  Actor and critic
are `mlp(cat([self_obs, eval_task(task_obs)]))`.

Departure from the reference, on purpose: it sizes the actor / critic input as `self_obs + task_mlp.units[-1] + 20`, the 20 being
its 10 path samples written as a literal (:32).  Here the width is `self_obs + task_mlp.units[-1] + detail['traj']` -- 368 + 256 + 30
= 654 with this repository's 15 samples, and the reference's number at its 10.  A trunk whose output width is not
`task_mlp.units[-1]` is refused at construction.

Where it runs: on a CUDA tensor the trunk is one `emloco_cnn_trunk` launch (normalisation switched off: like the reference's, the
module takes normalised observations) and every Linear one `emloco_gemm_f32` launch (`ops.linear`).  With grad enabled the device
trunk raises unless `enable_trunk_backward()` was called (AMPAgent does, run.py --train_policy --cnn_backward); then it goes through
`CnnTrunkFn`: the forward saves the map and the packed parameters and nothing else, the backward recomputes the activations on chip
and returns the weight and bias gradients (none for the map: observations are data).  In train mode RunningMeanStd updates its
statistics, so the training module keeps taking normalised rows (the fused normalisation is the frozen runner's).  On a CPU tensor,
where no kernel of this package can run, the same layers are evaluated by torch (host tests build the module and compare it with the
reference's fixtures that way)."""
import ctypes as C
import math

import torch
import torch.nn as nn

from ..predictor import ops
from .amp_network_sept_builder import AMPSeptBuilder, _ACTIVATIONS, _Head, _initializer, build_mlp

_CNN_MLP_UNITS = (512, 256)                   # amp_network_sept_cnn_builder.py:154, fixed in the reference's code
MAX_LAYERS, MAX_FILTERS = 4, 16               # what emloco_cnn_trunk takes (csrc/cnn_kernels.hip)


def check_convs(cnn):
    """The `task_cnn` block the kernel serves: 1 to 4 conv2d layers of kernel 4 / stride 2 / padding 1 with at most 16 filters each."""
    if cnn.get("type") != "conv2d":
        raise NotImplementedError(f"task_cnn.type '{cnn.get('type')}' is not built (only conv2d; network_builder.py:125-133)")
    if _ACTIVATIONS.get(cnn.get("activation")) is not nn.ReLU:
        raise NotImplementedError(f"task_cnn.activation '{cnn.get('activation')}' is not built (the trunk kernel applies ReLU)")
    convs = cnn.get("convs") or []
    ok = 1 <= len(convs) <= MAX_LAYERS and all(
        c.get("kernel_size") == 4 and c.get("strides") == 2 and c.get("padding") == 1 and 1 <= int(c.get("filters", 0)) <= MAX_FILTERS for c in convs)
    if not ok:
        raise NotImplementedError(f"task_cnn.convs {convs} is not built: the trunk kernel takes 1 to {MAX_LAYERS} layers of kernel_size 4 / "
                                  f"strides 2 / padding 1 with at most {MAX_FILTERS} filters")
    return [int(c["filters"]) for c in convs]


def map_shape(detail, layers):
    """(res, channels) of the map in the task observation (amp_network_sept_cnn_builder.py:121-128)"""
    if "heightmap" in detail:
        width, channels = int(detail["heightmap"]), 1
    elif "heightmap_velocity" in detail:
        width, channels = int(detail["heightmap_velocity"]), 3
    else:
        raise NotImplementedError("the CNN network needs a 'heightmap' or 'heightmap_velocity' block in the task observation")
    res = math.isqrt(width // channels)
    if res * res * channels != width:
        raise NotImplementedError(f"the map of {width} values with {channels} channel(s) is not square")
    if res % (1 << layers) or res % 8 or res > 64:
        raise NotImplementedError(f"a map side of {res} does not halve cleanly through {layers} layers of the trunk kernel (a multiple of 8 and of "
                                  f"2^layers, at most 64)")
    return res, channels


def pack_trunk(convs):
    """The `params` operand of emloco_cnn_trunk from an nn.Sequential of Conv2d / ReLU: weights then bias of every layer, back to back."""
    return torch.cat([t.detach().reshape(-1).float() for m in convs if isinstance(m, nn.Conv2d) for t in (m.weight, m.bias)]).contiguous()


def cnn_trunk(x, col0, res, channels, filters, params, out, out_off=0, mean=None, var=None, eps=1e-5, clip=5.0):
    """One emloco_cnn_trunk launch: the map at columns [col0, col0 + channels * res^2) of the rows x (fp32, on the device) -> features at
    columns [out_off, ...) of `out`.  mean / var (fp32, the map's columns only) switch the normalisation on."""
    lib = ops._lib()
    assert x.dtype == torch.float32 and x.stride(1) == 1 and out.dtype == torch.float32 and out.stride(1) == 1 and x.shape[0] == out.shape[0]
    f4 = list(filters) + [0] * (4 - len(filters))
    norm = mean is not None
    rc = lib.emloco_cnn_trunk(x.shape[0], res, channels, len(filters), *f4, ops._p(x, col0), x.stride(0), ops._p(mean) if norm else None,
                              ops._p(var) if norm else None, C.c_float(eps), C.c_float(clip), int(norm), ops._p(params), ops._p(out),
                              out.stride(0), out_off, ops._st(x))
    ops._chk(rc, "emloco_cnn_trunk")
    return out


def cnn_trunk_backward(x, col0, res, channels, filters, params, dout, dout_off=0, mean=None, var=None, eps=1e-5, clip=5.0):
    """One emloco_cnn_trunk_backward call (two launches on x's current stream): the operands of `cnn_trunk` and `dout`, the gradient of
    the features at columns [dout_off, ...) of its rows -> `dparams`, laid out like `params`: every weight and bias gradient summed
    over the rows.  The workspace is a fresh tensor per call (the trunk is evaluated on the actor's stream and on the critic's); no
    host synchronisation, so it may run inside a captured graph."""
    lib = ops._lib()
    assert x.dtype == torch.float32 and x.stride(1) == 1 and dout.dtype == torch.float32 and dout.stride(1) == 1 and x.shape[0] == dout.shape[0]
    assert params.dtype == torch.float32 and params.is_contiguous()
    f4 = list(filters) + [0] * (4 - len(filters))
    norm = mean is not None
    n_ws = lib.emloco_cnn_trunk_backward_workspace(x.shape[0], res, channels, len(filters), *f4)
    ops._chk(-1 if n_ws < 0 else 0, "emloco_cnn_trunk_backward_workspace")
    workspace = torch.empty(n_ws, dtype=torch.float32, device=x.device)
    dparams = torch.empty_like(params)
    rc = lib.emloco_cnn_trunk_backward(x.shape[0], res, channels, len(filters), *f4, ops._p(x, col0), x.stride(0), ops._p(mean) if norm else None,
                                       ops._p(var) if norm else None, C.c_float(eps), C.c_float(clip), int(norm), ops._p(params), ops._p(dout),
                                       dout.stride(0), dout_off, ops._p(dparams), ops._p(workspace), n_ws, ops._st(x))
    ops._chk(rc, "emloco_cnn_trunk_backward")
    return dparams


class CnnTrunkFn(torch.autograd.Function):
    """features = trunk(maps; w1, b1, w2, b2, ...) on the device, differentiable in the weights and biases: forward one `emloco_cnn_trunk`
    launch, backward one `emloco_cnn_trunk_backward` call that recomputes the activations on chip (nothing but the map and the packed
    parameters is saved).  The map gets no gradient -- the observations are data -- and one that asks for it is refused."""

    @staticmethod
    def forward(ctx, maps, res, channels, filters, *wb):
        if maps.requires_grad:
            raise NotImplementedError("CnnTrunkFn: `maps` requires grad, and the trunk's backward produces no gradient with respect to the map")
        assert len(wb) == 2 * len(filters)
        params = torch.cat([t.detach().reshape(-1).float() for t in wb]).contiguous()
        side = res >> len(filters)
        out = torch.empty((maps.shape[0], filters[-1] * side * side), dtype=torch.float32, device=maps.device)
        cnn_trunk(maps, 0, res, channels, filters, params, out)
        ctx.save_for_backward(maps, params)
        ctx.shape = (res, channels, tuple(filters))
        ctx.sizes = [(t.numel(), t.shape) for t in wb]
        return out

    @staticmethod
    def backward(ctx, dout):
        maps, params = ctx.saved_tensors
        res, channels, filters = ctx.shape
        dparams = cnn_trunk_backward(maps, 0, res, channels, filters, params, dout if dout.stride(1) == 1 else dout.contiguous())
        grads, at = [], 0
        for i, (n, shape) in enumerate(ctx.sizes):
            grads.append(dparams[at:at + n].view(shape) if ctx.needs_input_grad[4 + i] else None)
            at += n
        return (None, None, None, None, *grads)


class AMPSeptCNNBuilder:
    def __init__(self, **kwargs):
        self.params = None

    def load(self, params):
        self.params = params

    def build(self, name, **kwargs):
        return AMPSeptCNNBuilder.Network(self.params, **kwargs)

    def __call__(self, name, **kwargs):
        return self.build(name, **kwargs)

    class Network(AMPSeptBuilder.Network):
        def load(self, params):
            super().load(params)
            if params.get("normalization") is not None:
                raise NotImplementedError(f"normalization '{params['normalization']}' is not built (the shipped config has none)")
            if "task_cnn" not in params:
                raise NotImplementedError("the amp_sept_cnn network needs a task_cnn block")
            self._task_cnn = params["task_cnn"]
            self._filters = check_convs(self._task_cnn)

        def _mlp_input_size(self):
            # the reference: self_obs + task_mlp.units[-1] + 20 (:32); the 20 is its path width (module docstring)
            return self.self_obs_size + self._task_units[-1] + int(self.task_obs_size_detail["traj"])

        # (the parent's hook for its task MLP: this network has none)
        def _build_task_mlp(self):
            detail = self.task_obs_size_detail
            assert "traj" in detail
            if "people" in detail:
                raise NotImplementedError("the amp_sept_cnn network does not read a 'people' block (group_obs): its map slice assumes the map "
                                          "ends the row.  The people block is read by the amp_sept network's point-net branch")
            self.res, self.channels = map_shape(detail, len(self._filters))
            side = self.res >> len(self._filters)
            self.features = self._filters[-1] * side * side
            self.has_cnn_mlp = self.res != 32                               # :151
            trunk_out = _CNN_MLP_UNITS[-1] if self.has_cnn_mlp else self.features
            if trunk_out != self._task_units[-1]:
                raise NotImplementedError(f"the CNN trunk gives {trunk_out} features per row, task_mlp.units[-1] is {self._task_units[-1]}: the "
                                          "actor and critic inputs are sized by the latter, the two must be equal")
            # Conv2d layers keep torch's default initialisation, biases included: the reference builds them after its initialiser loop
            # (network_builder.py:262-270 runs inside super().__init__) and never reads task_cnn.initializer
            self._task_actor_cnn = self._build_conv()
            if self.has_cnn_mlp:
                # :152-158; the reference's `int((res / 32) ** 2 * 256)` is the three-layer 16-filter width, this is the trunk's own
                self._cnn_mlp = build_mlp(self.features, list(_CNN_MLP_UNITS), self._disc_activation)
            if self.separate:
                # built and never evaluated: the reference's eval_critic calls eval_task, which runs `_task_actor_cnn` (:69-83, :62).
                # The parameters are kept so that its checkpoints load with strict=True
                self._task_critic_cnn = self._build_conv()

        def _build_conv(self):
            layers, cin = [], self.channels
            for f in self._filters:
                layers += [nn.Conv2d(cin, f, kernel_size=4, stride=2, padding=1), nn.ReLU()]
                cin = f
            return nn.Sequential(*layers)

        _trunk_backward = False                                             # (a class default: `load` / `_build_task_mlp` run inside __init__)

        def enable_trunk_backward(self, on=True):
            """Opt in to (or out of) differentiating the device trunk: with grad enabled `_trunk` then goes through `CnnTrunkFn`
            instead of raising.  Off at construction.  The trunk's gradients reach the parameters through autograd's accumulation
            (not `ops.mark_direct_grad`): the trunk is evaluated on the actor's stream and on the critic's."""
            self._trunk_backward = bool(on)
            return self

        # ------------------------------------------------------------------ forward pieces
        def _trunk(self, maps):
            """(B, channels * res^2) normalised map columns, channel last -> (B, features), flattened (channel, row, column)"""
            if not maps.is_cuda:
                x = maps.reshape(maps.shape[0], self.res, self.res, self.channels).permute(0, 3, 1, 2)
                return self._task_actor_cnn(x).reshape(maps.shape[0], -1)
            if torch.is_grad_enabled():
                if not self._trunk_backward:
                    raise NotImplementedError("the CNN trunk's backward is not built into this module's default path: call "
                                              "enable_trunk_backward() to differentiate the device trunk (emloco_cnn_trunk_backward)")
                convs = [m for m in self._task_actor_cnn if isinstance(m, nn.Conv2d)]
                return CnnTrunkFn.apply(maps, self.res, self.channels, tuple(self._filters), *[t for m in convs for t in (m.weight, m.bias)])
            out = torch.empty((maps.shape[0], self.features), dtype=torch.float32, device=maps.device)
            return cnn_trunk(maps, 0, self.res, self.channels, self._filters, pack_trunk(self._task_actor_cnn), out)

        def eval_task(self, task_obs):                                      # (`_on`: the parent's)
            traj = int(self.task_obs_size_detail["traj"])
            maps = task_obs[:, traj:]
            feat = self._trunk(maps if maps.stride(1) == 1 else maps.contiguous())
            if self.has_cnn_mlp:
                feat = self._on(task_obs, self._cnn_mlp, feat)
            return torch.cat([feat, task_obs[:, :traj]], dim=-1)

        def eval_critic(self, obs):
            self_obs, task_obs = self._split(obs)
            c_input = torch.cat([self_obs, self.eval_task(task_obs)], dim=-1)
            return self.value_act(self._on(obs, self.value, self._on(obs, self.critic_mlp, c_input)))

        def eval_actor(self, obs):
            self_obs, task_obs = self._split(obs)
            actor_input = torch.cat([self_obs, self.eval_task(task_obs)], dim=-1)
            mu = self.mu_act(self._on(obs, self.mu, self._on(obs, self.actor_mlp, actor_input)))
            sigma = mu * 0.0 + self.sigma_act(self.sigma)
            return mu, sigma

        def eval_disc(self, amp_obs):
            return self._on(amp_obs, self._disc_logits, self._on(amp_obs, self._disc_mlp, amp_obs))
