"""What the fronts of the observation-batch entry points share (features.py, memory.py, q_targets.py, symmetry.py, and the
slots of selfplay_env.py): a batch of nine-plane observations (symmetry.py: of P planes), rows flattened, read in place when
the rows have one common stride.
Small checks that each caller composes in its own order; every one raises before anything touches a device."""

MAX_DIM = 32          # GVEC_MAX_DIM


def check_cap(cap):
    """cap as an int, or ValueError: a power of two in [2, 1024] (what makes every output value an exact float32)."""
    if isinstance(cap, bool) or not isinstance(cap, int):
        raise TypeError(f"cap must be an int, not {type(cap).__name__}")
    if cap < 2 or cap > 1024 or cap & (cap - 1):
        raise ValueError(f"cap must be a power of two in [2, 1024], not {cap}")
    return cap


def check_board(W, H):
    if not (1 <= W <= MAX_DIM and 1 <= H <= MAX_DIM):
        raise ValueError(f"board {W}x{H}: width and height must be in [1, {MAX_DIM}]")


def check_tensor(t, name, dtypes):
    """TypeError unless the argument `name` is a tensor of one of `dtypes` (None: of any floating-point dtype)"""
    import torch
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, not {type(t).__name__}")
    if dtypes is None:
        if not t.is_floating_point():
            raise TypeError(f"{name} must be a floating-point tensor, not {t.dtype}")
    elif t.dtype not in dtypes:
        raise TypeError(f"{name} must be {' or '.join(str(d).replace('torch.', '') for d in dtypes)}, not {t.dtype}")


def read_shape(obs, name, width=None, height=None):
    """(leading shape, rows, H, W) of observations [..., 9, H, W] - with width and height: [..., 9, H * W] - or ValueError"""
    if width is None:
        if obs.dim() < 3 or obs.shape[-3] != 9:
            raise ValueError(f"{name} {tuple(obs.shape)} is not [..., 9, H, W]")
        H, W = int(obs.shape[-2]), int(obs.shape[-1])
        lead = tuple(obs.shape[:-3])
    else:
        W, H = int(width), int(height)
        if obs.dim() < 2 or obs.shape[-2] != 9 or obs.shape[-1] != W * H:
            raise ValueError(f"{name} {tuple(obs.shape)} is not [..., 9, {H} * {W}]")
        lead = tuple(obs.shape[:-2])
    check_board(W, H)
    rows = 1
    for d in lead:
        rows *= int(d)
    return lead, rows, H, W


def check_device(what, first, **tensors):
    """Every tensor given (None: skipped) is on the CUDA device of the first, the argument named `first`; returns that
    device.  `what` is the caller's own wording of who computes there."""
    dev = None
    for name, t in tensors.items():
        if t is None:
            continue
        if not t.is_cuda:
            raise ValueError(f"{name} must be a CUDA tensor: {what} (there is no host path)")
        dev = dev or t.device
        if t.device != dev:
            raise ValueError(f"{name} is on {t.device}, {first} on {dev}")
    return dev


def row_stride(obs, tail, row_floats):
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


def in_place(obs, tail, H, W):
    """(obs to read, its row stride in floats): obs itself where its rows have one common stride, else a contiguous copy"""
    return in_place_planes(obs, tail, 9, H, W)


def in_place_planes(t, tail, P, H, W):
    """in_place for rows of P planes: [..., P, H, W] (tail 3) or [..., P, H * W] (tail 2)"""
    t = t.detach()
    if t.is_contiguous():                            # the common case, without walking the strides
        return t, P * W * H
    stride = row_stride(t, tail, P * W * H)
    return (t, stride) if stride is not None else (t.contiguous(), P * W * H)


def read_plane_shape(t, name, max_planes):
    """(leading shape, rows, P, H, W) of planes [..., P, H, W] with 1 <= P <= max_planes, or ValueError"""
    if t.dim() < 3 or not 1 <= t.shape[-3] <= max_planes:
        raise ValueError(f"{name} {tuple(t.shape)} is not [..., P, H, W] with P in [1, {max_planes}]")
    P, H, W = int(t.shape[-3]), int(t.shape[-2]), int(t.shape[-1])
    lead = tuple(t.shape[:-3])
    check_board(W, H)
    rows = 1
    for d in lead:
        rows *= int(d)
    return lead, rows, P, H, W


def check_out(out, name, dtypes, dtype_words, numel, dev):
    """`out` where a launch may write numel elements of one of `dtypes` (in the message: dtype_words), or ValueError"""
    import torch
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == dev and out.dtype in dtypes and out.is_contiguous()
            and out.numel() == numel):
        raise ValueError(f"{name} must be a contiguous {dtype_words} CUDA tensor of {numel} elements on {dev}")
    return out


def stream(dev):
    import torch
    return torch.cuda.current_stream(dev).cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()
