"""MaskedCategoricalHead — the action step of on-device PPO: logits [..., A] and the env's legal-action mask in, an action,
its log-probability and the entropy out, and the same distribution evaluated (with gradients) in the update.

Three HIP entry points do the work (include/generals_vec.h): gvec_policy_sample (Gumbel-max on the
build's counter RNG, or greedy), gvec_policy_evaluate, gvec_policy_backward.  One wavefront per row, each row read from HBM
once; no [rows, A] tensor is saved between forward and backward.  A row without a legal action (an eliminated learner of
GeneralsSelfPlayVecEnv) gives action 0, logp 0, entropy 0 and zero gradients - never a NaN.

    head = MaskedCategoricalHead()
    actions, logp, entropy = head.sample(policy_logits, buf.valid_actions_mask, seed=step)      # [B, L] each
    new_logp, entropy = head.evaluate(policy_logits, batch["valid_actions_mask"], batch["action"])

Two more train the same logits on a search's policy target: gvec_policy_distill and
gvec_policy_distill_backward, the masked soft-target cross-entropy / KL and its gradient, sharing the rows' code and rounding.

    ce, kl, entropy = head.distill(policy_logits, batch["valid_actions_mask"], batch["policy_target"])
    loss = distill_loss(policy_logits, batch["valid_actions_mask"], batch["policy_target"], batch["weight"])

Everything runs on the current torch stream; nothing synchronises with the host.
"""
import ctypes as C

from ._lib import (GvecError, PolicyBackwardArgs, PolicyDistillArgs, PolicyDistillBackwardArgs, PolicyEvaluateArgs, PolicySampleArgs,
                   check, load)


class MaskedCategoricalHead:
    def __init__(self, device=None):
        import torch
        if not torch.cuda.is_available():
            raise GvecError(-2, "MaskedCategoricalHead needs a GPU: sampling, evaluation and the gradient are HIP kernels "
                                "(there is no host path)")
        self._t = t = torch
        if device is None:
            device = torch.cuda.current_device()
        if isinstance(device, torch.device):
            device = torch.cuda.current_device() if device.index is None else device.index
        self._dev = dev = torch.device("cuda", int(device))
        self._L = L = load()
        self._bad = bad = torch.zeros(1, dtype=torch.int64, device=dev)
        stream = lambda: t.cuda.current_stream(dev).cuda_stream

        class _Evaluate(torch.autograd.Function):
            @staticmethod
            def forward(ctx, logits, mask, actions):
                rows, A = logits.shape
                logp, ent = t.empty(rows, dtype=t.float32, device=dev), t.empty(rows, dtype=t.float32, device=dev)
                a = PolicyEvaluateArgs(rows=rows, num_actions=A, logits=logits.data_ptr(), mask=mask.data_ptr(), action=actions.data_ptr(),
                                       logp=logp.data_ptr(), entropy=ent.data_ptr(), bad_actions=bad.data_ptr())
                check(L.gvec_policy_evaluate(dev.index, stream(), C.byref(a)), "gvec_policy_evaluate")
                ctx.save_for_backward(logits, mask, actions)   # the inputs themselves: p is recomputed from them
                return logp, ent

            @staticmethod
            def backward(ctx, grad_logp, grad_entropy):
                logits, mask, actions = ctx.saved_tensors
                rows, A = logits.shape
                f32 = lambda g: None if g is None else g.to(dtype=t.float32).contiguous()
                gl, ge = f32(grad_logp), f32(grad_entropy)
                grad = t.empty_like(logits)                    # every element is written by the kernel
                a = PolicyBackwardArgs(rows=rows, num_actions=A, logits=logits.data_ptr(), mask=mask.data_ptr(), action=actions.data_ptr(),
                                       grad_logp=None if gl is None else gl.data_ptr(),
                                       grad_entropy=None if ge is None else ge.data_ptr(), grad_logits=grad.data_ptr())
                check(L.gvec_policy_backward(dev.index, stream(), C.byref(a)), "gvec_policy_backward")
                return grad, None, None

        self._evaluate = _Evaluate

        class _Distill(torch.autograd.Function):
            @staticmethod
            def forward(ctx, logits, mask, target):
                rows, A = logits.shape
                ce, kl, ent = (t.empty(rows, dtype=t.float32, device=dev) for _ in range(3))
                a = PolicyDistillArgs(rows=rows, num_actions=A, logits=logits.data_ptr(), mask=mask.data_ptr(), target=target.data_ptr(),
                                      ce=ce.data_ptr(), kl=kl.data_ptr(), entropy=ent.data_ptr())
                check(L.gvec_policy_distill(dev.index, stream(), C.byref(a)), "gvec_policy_distill")
                ctx.save_for_backward(logits, mask, target)    # the inputs themselves: p and tau are recomputed from them
                return ce, kl, ent

            @staticmethod
            def backward(ctx, grad_ce, grad_kl, grad_entropy):
                logits, mask, target = ctx.saved_tensors
                rows, A = logits.shape
                f32 = lambda g: None if g is None else g.to(dtype=t.float32).contiguous()
                gc, gk, ge = f32(grad_ce), f32(grad_kl), f32(grad_entropy)
                ptr = lambda g: None if g is None else g.data_ptr()
                grad = t.empty_like(logits)                    # every element is written by the kernel
                a = PolicyDistillBackwardArgs(rows=rows, num_actions=A, logits=logits.data_ptr(), mask=mask.data_ptr(),
                                              target=target.data_ptr(), grad_ce=ptr(gc), grad_kl=ptr(gk), grad_entropy=ptr(ge),
                                              grad_logits=grad.data_ptr())
                check(L.gvec_policy_distill_backward(dev.index, stream(), C.byref(a)), "gvec_policy_distill_backward")
                return grad, None, None                        # the target is a constant

        self._distill = _Distill

    @property
    def bad_actions(self):
        """How many actions `evaluate` has met that were out of range or not legal in their (live) row: those rows got logp 0
        and no logp gradient.  A device counter; reading it here is the one host sync of this class."""
        return int(self._bad.item())

    def _as(self, x, dtype, shape):
        t = self._t
        if not isinstance(x, t.Tensor):
            x = t.as_tensor(x)
        if x.dtype == t.bool and dtype == t.uint8:
            x = x.contiguous().view(t.uint8)
        if not (x.is_cuda and x.device == self._dev and x.dtype == dtype and x.is_contiguous()):
            x = x.to(device=self._dev, dtype=dtype).contiguous()       # differentiable where x carries a graph
        return x.reshape(shape)

    def _rows(self, logits, mask):
        lead, A = tuple(logits.shape[:-1]), int(logits.shape[-1])
        if tuple(mask.shape) != tuple(logits.shape):
            raise ValueError(f"mask {tuple(mask.shape)} and logits {tuple(logits.shape)} must have the same shape")
        rows = 1
        for d in lead:
            rows *= int(d)
        return lead, rows, A

    def sample(self, logits, mask, seed, row_base=0, greedy=False):
        """logits float32 [..., A], mask bool / uint8 [..., A] (CUDA, contiguous: anything else is converted first).  Returns
        (action int64, logp float32, entropy float32), each of the leading shape.  The draw of row r, element i depends on
        (seed, row_base + r, i) alone: give every step its own seed."""
        t = self._t
        with t.no_grad():
            lead, rows, A = self._rows(logits, mask)
            logits, mask = self._as(logits, t.float32, (rows, A)), self._as(mask, t.uint8, (rows, A))
            e = lambda dt: t.empty(rows, dtype=dt, device=self._dev)
            action, logp, ent = e(t.int64), e(t.float32), e(t.float32)
            a = PolicySampleArgs(rows=rows, num_actions=A, greedy=1 if greedy else 0, seed=int(seed) & (2 ** 64 - 1), row_base=int(row_base),
                                 logits=logits.data_ptr(), mask=mask.data_ptr(), action=action.data_ptr(), logp=logp.data_ptr(),
                                 entropy=ent.data_ptr())
            check(self._L.gvec_policy_sample(self._dev.index, t.cuda.current_stream(self._dev).cuda_stream, C.byref(a)),
                  "gvec_policy_sample")
            return action.view(lead), logp.view(lead), ent.view(lead)

    def evaluate(self, logits, mask, actions):
        """(logp of actions, entropy), each of the leading shape of logits [..., A]; differentiable with respect to logits
        (the backward is gvec_policy_backward).  actions int64 [...]."""
        t = self._t
        lead, rows, A = self._rows(logits, mask)
        logits, mask = self._as(logits, t.float32, (rows, A)), self._as(mask, t.uint8, (rows, A))
        actions = self._as(actions, t.int64, (rows,))
        if rows == 0:
            z = logits.sum(-1)
            return z.view(lead), z.view(lead)
        logp, ent = self._evaluate.apply(logits, mask, actions)
        return logp.view(lead), ent.view(lead)

    def distill(self, logits, mask, target):
        """(ce, kl, entropy) of logits [..., A] against a soft target, each of the leading shape; differentiable with respect
        to logits (the backward is gvec_policy_distill_backward), the target gets no gradient.  target: float32 of the shape
        of logits, what HalvingSearch.policy_target / SelfPlayRolloutBuffer.gather return; it need not be normalised, and
        mass on illegal actions, negative and NaN entries are dropped.  ce = -sum tau_i logp_i, kl = sum tau_i (log tau_i -
        logp_i); a row without a legal action gives zeros and a zero gradient."""
        _check_distill_inputs(logits, mask, target)            # a ValueError before any library call
        t = self._t
        lead, rows, A = self._rows(logits, mask)
        logits, mask = self._as(logits, t.float32, (rows, A)), self._as(mask, t.uint8, (rows, A))
        target = self._as(target.detach(), t.float32, (rows, A))
        if rows == 0:
            z = logits.sum(-1)
            return z.view(lead), z.view(lead), z.view(lead)
        ce, kl, ent = self._distill.apply(logits, mask, target)
        return ce.view(lead), kl.view(lead), ent.view(lead)


def _check_distill_inputs(logits, mask, target):
    import torch
    for name, x in (("logits", logits), ("mask", mask), ("target", target)):
        if not isinstance(x, torch.Tensor):
            raise ValueError(f"distill: {name} must be a torch tensor, not {type(x).__name__}")
    if logits.dim() < 1:
        raise ValueError("distill: logits must be [..., A]")
    if tuple(mask.shape) != tuple(logits.shape):
        raise ValueError(f"mask {tuple(mask.shape)} and logits {tuple(logits.shape)} must have the same shape")
    if tuple(target.shape) != tuple(logits.shape):
        raise ValueError(f"target {tuple(target.shape)} and logits {tuple(logits.shape)} must have the same shape")
    if target.dtype != torch.float32:
        raise ValueError(f"target must be float32, not {target.dtype}")


_heads = {}


def distill_loss(logits, mask, target, weight=None):
    """The policy loss of search distillation: the `weight`-weighted mean over rows of MaskedCategoricalHead.distill's ce,
    sum(weight * ce) / max(sum(weight), 1); weight None counts every row once.  `weight` is of the leading shape of logits
    (SelfPlayRolloutBuffer.gather's batch["weight"]: 0 on rejected positions)."""
    import torch
    _check_distill_inputs(logits, mask, target)
    if weight is not None and tuple(weight.shape) != tuple(logits.shape[:-1]):
        raise ValueError(f"weight {tuple(weight.shape)} must have the leading shape {tuple(logits.shape[:-1])} of logits")
    index = logits.device.index if logits.is_cuda else None    # elsewhere: the current device, as MaskedCategoricalHead() takes it
    if index is None and torch.cuda.is_available():
        index = torch.cuda.current_device()
    head = _heads.get(index)
    if head is None:
        head = MaskedCategoricalHead(index)                    # raises without a GPU: there is no host path
        _heads[index] = head
    ce, _, _ = head.distill(logits, mask, target)
    if weight is None:
        return ce.sum() / max(ce.numel(), 1)
    w = weight.to(device=ce.device, dtype=torch.float32)
    return (w * ce).sum() / w.sum().clamp(min=1.0)
