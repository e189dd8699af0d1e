"""strategic_features — five planes next to the nine of an observation that a small conv torso cannot compute for itself:
capped shortest-path distances to the own general, to the nearest enemy tile the observation shows, to the nearest city
still to take and to the nearest fogged tile, and the front line (include/generals_vec.h "strategic feature planes",
DESIGN.md section 4.13).

A pure function of the observation: it shows the learner nothing the nine planes did not already show, and it works on any
batch of them - what `step` just returned, a DeviceReplayBuffer / sample_nstep batch, a SelfPlayRolloutBuffer minibatch.
Stores keep nine planes per row; the features are recomputed where they are consumed.

    feats = strategic_features(obs)                      # [..., 9, H, W] -> [..., 5, H, W]
    x = torch.cat([obs, feats], dim=-3)                  # a 14-channel torso input

One HIP launch (gvec_obs_features: one wavefront per observation, a bit-plane breadth-first search) on the current torch
stream; nothing synchronises with the host.
"""
import ctypes as C

from ._lib import ObsFeaturesArgs, check, load

NUM_STRATEGIC_FEATURES = 5
STRATEGIC_FEATURE_NAMES = ("dist_own_general", "dist_enemy", "dist_city", "dist_fog", "front_line")
MAX_DIM = 32          # GVEC_MAX_DIM


def check_cap(cap):
    """cap as an int, or ValueError: a power of two in [2, 1024] (what makes every output value an exact float32)."""
    if isinstance(cap, bool) or not isinstance(cap, int):
        raise TypeError(f"cap must be an int, not {type(cap).__name__}")
    if cap < 2 or cap > 1024 or cap & (cap - 1):
        raise ValueError(f"cap must be a power of two in [2, 1024], not {cap}")
    return cap


def strategic_features(obs, cap=64, out=None, width=None, height=None):
    """obs: CUDA float32 tensor [..., 9, H, W], or [..., 9, H * W] with width= and height=.  Returns float32
    [..., 5, H, W] (or [..., 5, H * W]): planes STRATEGIC_FEATURE_NAMES, distances as min(d, cap) / cap.

    Leading dimensions are flattened.  No copy is made when the planes of an observation are contiguous and the leading
    dimensions have one common stride (a slice of a larger row, a rollout slot); otherwise obs.contiguous() is used.
    out: a contiguous float32 CUDA tensor with the result's number of elements to write into (every element is written).
    The features are not differentiable with respect to obs: the result carries no autograd graph.
    ValueError / TypeError before any launch: a CPU tensor, another dtype, a plane count other than 9, a bad cap."""
    import torch
    cap = check_cap(cap)
    if not isinstance(obs, torch.Tensor):
        raise TypeError(f"obs must be a torch.Tensor, not {type(obs).__name__}")
    if obs.dtype != torch.float32:
        raise TypeError(f"obs must be float32, not {obs.dtype}")
    if not obs.is_cuda:
        raise ValueError("obs must be a CUDA tensor: the features are computed by a HIP kernel (there is no host path)")
    flat = width is not None or height is not None
    if flat:
        if width is None or height is None:
            raise ValueError("width and height go together")
        W, H = int(width), int(height)
        if obs.dim() < 2 or obs.shape[-2] != 9 or obs.shape[-1] != W * H:
            raise ValueError(f"obs {tuple(obs.shape)} is not [..., 9, {H} * {W}]")
        lead, tail = tuple(obs.shape[:-2]), 2
    else:
        if obs.dim() < 3 or obs.shape[-3] != 9:
            raise ValueError(f"obs {tuple(obs.shape)} is not [..., 9, H, W]")
        H, W = int(obs.shape[-2]), int(obs.shape[-1])
        lead, tail = tuple(obs.shape[:-3]), 3
    if not (1 <= W <= MAX_DIM and 1 <= H <= MAX_DIM):
        raise ValueError(f"board {W}x{H}: width and height must be in [1, {MAX_DIM}]")
    rows = 1
    for d in lead:
        rows *= int(d)
    out_shape = lead + ((5, W * H) if flat else (5, H, W))
    obs = obs.detach()
    stride = _row_stride(obs, tail, 9 * W * H)
    if stride is None:
        obs = obs.contiguous()
        stride = 9 * W * H
    if out is None:
        out = torch.empty(out_shape, dtype=torch.float32, device=obs.device)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == obs.device and out.dtype == torch.float32
              and out.is_contiguous() and out.numel() == rows * 5 * W * H):
        raise ValueError(f"out must be a contiguous float32 CUDA tensor of {rows * 5 * W * H} elements on {obs.device}")
    if rows:
        a = ObsFeaturesArgs(rows=rows, width=W, height=H, cap=cap, reserved=0, obs_row_stride=stride, obs=obs.data_ptr(),
                            out=out.data_ptr())
        check(load().gvec_obs_features(obs.device.index, torch.cuda.current_stream(obs.device).cuda_stream, C.byref(a)),
              "gvec_obs_features")
    return out.view(out_shape)


def _row_stride(obs, tail, row_floats):
    """Floats between consecutive observations when obs can be read in place, else None."""
    shape, strides = tuple(obs.shape), tuple(obs.stride())
    expect = 1
    for n, s in zip(reversed(shape[-tail:]), reversed(strides[-tail:])):      # the planes of one observation: dense
        if n != 1 and s != expect:
            return None
        expect *= n
    lead = [(n, s) for n, s in zip(shape[:-tail], strides[:-tail]) if n != 1]
    if not lead:
        return row_floats
    stride = lead[-1][1]
    if stride < row_floats:
        return None
    expect = stride
    for n, s in reversed(lead):                                                  # the leading dimensions: one common stride
        if s != expect:
            return None
        expect *= n
    return stride
