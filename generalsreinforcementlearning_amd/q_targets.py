"""q_targets — bootstrap targets over the LEGAL actions of the next state, from a replay batch that stores no mask
(include/generals_vec.h "masked Q targets").

The legal-action mask is a pure function of the observation (own tiles with an army above 1, neighbours that are no
mountain), so it is recomputed from `ns` where it is needed: on its own, inside the (Double) DQN target, inside the
categorical (C51) target.  Each is one HIP launch on the current torch stream, one wavefront per row; nothing synchronises
with the host, and the Q values or logits of illegal actions are never read.

    mask = valid_actions_mask_from_observation(ns)                                   # bool [..., 5 * H * W]
    tq, a_next = double_q_target(ns, target(ns), r, disc, d, q_select=q(ns))          # q_select=None: plain masked DQN
    m, a_next = categorical_target(ns, tgt_logits, r, disc, d, v_min, v_max, logits_select=onl_logits)    # [..., N]

The categorical loss stays in torch: gather the taken action's N logits, log_softmax, -(m * logp).sum(-1).
"""
import ctypes as C
import math

from . import _obs_batch as ob
from ._lib import CategoricalTargetArgs, ObsValidMaskArgs, QTargetArgs, check, load

MAX_ATOMS = 64        # one lane per atom


def _observations(obs, name):
    """(leading shape, rows, H, W) of observations [..., 9, H, W], or TypeError / ValueError"""
    import torch
    ob.check_tensor(obs, name, (torch.float32,))
    return ob.read_shape(obs, name)


def _same_device(obs_name, **tensors):
    """every tensor is on the CUDA device of the first (the observations): checked last, so that a CPU-only box still sees
    every other refusal"""
    return ob.check_device("the targets are computed by HIP kernels", obs_name, **tensors)


def _shaped(t, name, shape, dtypes):
    """checks the type, dtype (a tuple of dtypes, or None = any floating-point) and shape of one argument"""
    ob.check_tensor(t, name, dtypes)
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} {tuple(t.shape)} is not {tuple(shape)}")


def _per_row(reward, discount, done, lead):
    """checks the three per-row arguments; the discount as (tensor or None, scalar gamma)"""
    import torch
    _shaped(reward, "reward", lead, None)
    gamma = 0.0
    if isinstance(discount, torch.Tensor):
        _shaped(discount, "discount", lead, None)
    elif isinstance(discount, bool) or not isinstance(discount, (int, float)):
        raise TypeError(f"discount must be a float or a tensor, not {type(discount).__name__}")
    else:
        gamma, discount = float(discount), None
    _shaped(done, "done", lead, (torch.bool, torch.uint8))
    return discount, gamma


def _f32(t):
    import torch
    return None if t is None else t.detach().to(torch.float32).contiguous()


def _u8(done):
    import torch
    done = done.detach().contiguous()
    return done.view(torch.uint8) if done.dtype == torch.bool else done


def valid_actions_mask_from_observation(obs, out=None):
    """obs: CUDA float32 [..., 9, H, W].  Returns bool [..., 5 * H * W]: info["valid_actions_mask"] of the state the
    observation shows, byte for byte (action (y * W + x) * 5 + d; d = up, right, down, left, half).

    Leading dimensions are flattened; no copy is made when the planes of an observation are contiguous and the leading
    dimensions have one common stride, as for strategic_features.  out: a contiguous bool or uint8 CUDA tensor with the
    result's number of elements to write into (every element is written).
    ValueError / TypeError before any launch: a CPU tensor, another dtype, a plane count other than 9."""
    import torch
    lead, rows, H, W = _observations(obs, "obs")
    dev = _same_device("obs", obs=obs)
    obs, stride = ob.in_place(obs, 3, H, W)
    A = 5 * H * W
    if out is None:
        out = torch.empty(lead + (A,), dtype=torch.bool, device=dev)
    else:
        ob.check_out(out, "out", (torch.bool, torch.uint8), "bool or uint8", rows * A, dev)
    if rows:
        a = ObsValidMaskArgs(rows=rows, width=W, height=H, obs_row_stride=stride, obs=obs.data_ptr(), mask=out.data_ptr())
        check(load().gvec_obs_valid_mask(dev.index, ob.stream(dev), C.byref(a)), "gvec_obs_valid_mask")
    out = out.view(lead + (A,))
    return out if out.dtype == torch.bool else out.view(torch.bool)


def double_q_target(next_obs, q_eval, reward, discount, done, q_select=None, return_next_value=False):
    """The masked (Double) DQN target of a batch: a* = argmax over the LEGAL actions of next_obs of q_select (q_eval when
    q_select is None: plain masked DQN), target = reward + discount * q_eval[a*], and target = reward on done rows and on
    rows without a legal action.

    next_obs float32 [..., 9, H, W]; q_eval, q_select float32 [..., 5 * H * W] (the target and the online network's output for
    next_obs); reward any float dtype [...] (converted to float32); discount a float, or a tensor [...] (gamma ** steps of an
    n-step batch); done bool or uint8 [...].  Returns (target float32 [...], next_action int64 [...], -1 where no action is
    legal), and next_value = q_eval[a*] (0 where nothing is bootstrapped) as a third result with return_next_value=True.
    The results carry no autograd graph.  ValueError / TypeError before any launch: CPU tensors, wrong dtypes, shapes that
    disagree with the observation's 5 * H * W, a plane count other than 9."""
    import torch
    lead, rows, H, W = _observations(next_obs, "next_obs")
    A = 5 * H * W
    _shaped(q_eval, "q_eval", lead + (A,), (torch.float32,))
    if q_select is not None:
        _shaped(q_select, "q_select", lead + (A,), (torch.float32,))
    disc, gamma = _per_row(reward, discount, done, lead)
    dev = _same_device("next_obs", next_obs=next_obs, q_eval=q_eval, q_select=q_select, reward=reward, discount=disc, done=done)
    obs, stride = ob.in_place(next_obs, 3, H, W)
    q_eval, q_select, reward, disc, done = _f32(q_eval), _f32(q_select), _f32(reward), _f32(disc), _u8(done)
    target = torch.empty(lead, dtype=torch.float32, device=dev)
    action = torch.empty(lead, dtype=torch.int64, device=dev)
    value = torch.empty(lead, dtype=torch.float32, device=dev) if return_next_value else None
    if rows:
        a = QTargetArgs(rows=rows, width=W, height=H, obs_row_stride=stride, gamma=gamma, reserved=0, next_obs=obs.data_ptr(),
                        q_eval=q_eval.data_ptr(), q_select=ob.ptr(q_select), reward=reward.data_ptr(), discount=ob.ptr(disc),
                        done=done.data_ptr(), target=target.data_ptr(), next_action=action.data_ptr(), next_value=ob.ptr(value))
        check(load().gvec_q_target(dev.index, ob.stream(dev), C.byref(a)), "gvec_q_target")
    return (target, action, value) if return_next_value else (target, action)


def check_support(num_atoms, v_min, v_max):
    """(num_atoms, v_min, v_max) as (int, float, float), or ValueError: 2 <= num_atoms <= 64, finite v_min < v_max."""
    if not 2 <= int(num_atoms) <= MAX_ATOMS:
        raise ValueError(f"num_atoms must be in [2, {MAX_ATOMS}], not {num_atoms}")
    v_min, v_max = float(v_min), float(v_max)
    if not (math.isfinite(v_min) and math.isfinite(v_max) and v_min < v_max):
        raise ValueError(f"v_min {v_min} and v_max {v_max} must be finite with v_min < v_max")
    return int(num_atoms), v_min, v_max


def categorical_target(next_obs, logits_eval, reward, discount, done, v_min, v_max, logits_select=None):
    """The projected categorical (C51) target of a batch.  With the support z_j = v_min + j * (v_max - v_min) / (N - 1): over
    the LEGAL actions i of next_obs, Q_i = sum_j softmax(logits_select[i])_j z_j (logits_eval when logits_select is None),
    a* = argmax Q_i, and m = the projection of softmax(logits_eval[a*]) moved to clamp(reward + discount * z, v_min, v_max)
    back onto the support.  A done row, and a row without a legal action, gives the projected point mass at the clamped reward
    (next_action -1; the logits of a done row are not read).

    logits_eval, logits_select float32 [..., 5 * H * W, N], atoms innermost (a non-contiguous tensor is copied: have the
    network produce this layout); 2 <= N <= 64.  reward, discount, done as for double_q_target.  Returns (m float32 [..., N],
    next_action int64 [...]) without an autograd graph.  ValueError / TypeError before any launch: CPU tensors, wrong dtypes,
    shapes that disagree with the observation's 5 * H * W, N outside [2, 64], v_min >= v_max or bounds that are not finite, a
    plane count other than 9."""
    import torch
    lead, rows, H, W = _observations(next_obs, "next_obs")
    A = 5 * H * W
    if not isinstance(logits_eval, torch.Tensor):
        raise TypeError(f"logits_eval must be a torch.Tensor, not {type(logits_eval).__name__}")
    if logits_eval.dim() != len(lead) + 2 or tuple(logits_eval.shape[:-1]) != lead + (A,):
        raise ValueError(f"logits_eval {tuple(logits_eval.shape)} is not {lead + (A, 'N')}")
    N, v_min, v_max = check_support(logits_eval.shape[-1], v_min, v_max)
    _shaped(logits_eval, "logits_eval", lead + (A, N), (torch.float32,))
    if logits_select is not None:
        _shaped(logits_select, "logits_select", lead + (A, N), (torch.float32,))
    disc, gamma = _per_row(reward, discount, done, lead)
    dev = _same_device("next_obs", next_obs=next_obs, logits_eval=logits_eval, logits_select=logits_select, reward=reward,
                       discount=disc, done=done)
    obs, stride = ob.in_place(next_obs, 3, H, W)
    logits_eval, logits_select, reward, disc, done = _f32(logits_eval), _f32(logits_select), _f32(reward), _f32(disc), _u8(done)
    m = torch.empty(lead + (N,), dtype=torch.float32, device=dev)
    action = torch.empty(lead, dtype=torch.int64, device=dev)
    if rows:
        a = CategoricalTargetArgs(rows=rows, width=W, height=H, obs_row_stride=stride, num_atoms=N, gamma=gamma, v_min=v_min,
                                  v_max=v_max, next_obs=obs.data_ptr(), logits_eval=logits_eval.data_ptr(),
                                  logits_select=ob.ptr(logits_select), reward=reward.data_ptr(), discount=ob.ptr(disc),
                                  done=done.data_ptr(), m=m.data_ptr(), next_action=action.data_ptr())
        check(load().gvec_categorical_target(dev.index, ob.stream(dev), C.byref(a)), "gvec_categorical_target")
    return m, action
