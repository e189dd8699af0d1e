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

from . import _obs_batch as ob
from ._lib import ObsFeaturesArgs, check, load

NUM_STRATEGIC_FEATURES = 5
STRATEGIC_FEATURE_NAMES = ("dist_own_general", "dist_enemy", "dist_city", "dist_fog", "front_line")


def strategic_features(obs, cap=64, out=None, width=None, height=None):
    """obs: CUDA float32 tensor [..., 9, H, W], or [..., 9, H * W] with width= and height=.  Returns float32
    [..., 5, H, W] (or [..., 5, H * W]): planes STRATEGIC_FEATURE_NAMES, distances as min(d, cap) / cap.

    Leading dimensions are flattened.  No copy is made when the planes of an observation are contiguous and the leading
    dimensions have one common stride (a slice of a larger row, a rollout slot); otherwise obs.contiguous() is used.
    out: a contiguous float32 CUDA tensor with the result's number of elements to write into (every element is written).
    The features are not differentiable with respect to obs: the result carries no autograd graph.
    ValueError / TypeError before any launch: a CPU tensor, another dtype, a plane count other than 9, a bad cap."""
    import torch
    cap = ob.check_cap(cap)
    ob.check_tensor(obs, "obs", (torch.float32,))
    # the device before the shape: a CPU tensor is refused as such
    dev = ob.check_device("the features are computed by a HIP kernel", "obs", obs=obs)
    flat = width is not None or height is not None
    if flat and (width is None or height is None):
        raise ValueError("width and height go together")
    lead, rows, H, W = ob.read_shape(obs, "obs", width, height)
    out_shape = lead + ((5, W * H) if flat else (5, H, W))
    obs, stride = ob.in_place(obs, 2 if flat else 3, H, W)
    if out is None:
        out = torch.empty(out_shape, dtype=torch.float32, device=dev)
    else:
        ob.check_out(out, "out", (torch.float32,), "float32", rows * 5 * W * H, dev)
    if rows:
        a = ObsFeaturesArgs(rows=rows, width=W, height=H, cap=cap, reserved=0, obs_row_stride=stride, obs=obs.data_ptr(),
                            out=out.data_ptr())
        check(load().gvec_obs_features(dev.index, ob.stream(dev), C.byref(a)), "gvec_obs_features")
    return out.view(out_shape)
