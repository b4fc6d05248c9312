"""The argument checks of Interpolator.update_points / update_permeability / update_neumann_flags, each written once.  A check raises
(TypeError for a kind or dtype that would need a silent cast, ValueError for a value, a shape or a device) or hands back the argument in
the form the native call takes; none of them has a side effect.  Where the copies these functions replace disagreed, the difference is a
parameter that says so ("as found"): nobody decided it, and a later change may."""
import numpy as np


def is_torch(a):
    return type(a).__module__.split(".")[0] == "torch"


def on_gpu(a):
    return is_torch(a) and getattr(a, "is_cuda", False)


def to_host(a):
    """A CPU torch tensor as the numpy array over its memory; anything else as it is."""
    return a.detach().numpy() if is_torch(a) else a


def _one_of(names):
    return names[0] if len(names) == 1 else ", ".join(names[:-1]) + " or " + names[-1]


def check_shape(shape, name, shapes):
    if tuple(shape) not in shapes:
        raise ValueError(f"{name} must have shape {' or '.join(map(str, shapes))}, not {tuple(shape)}")


def host_ids(ids, name, n, empty_of_any_dtype=False):
    """Ids on the host (an array or a list) as contiguous int64: integers, 1-D, all in [0, n).
    empty_of_any_dtype, as found: update_neumann_flags takes `[]` (numpy makes an empty list float64); update_points and
    update_permeability raise the TypeError for it."""
    ids = np.asarray(ids)
    if ids.dtype.kind not in "iu" and not (empty_of_any_dtype and ids.size == 0):
        raise TypeError(f"{name} must be integers, not {ids.dtype} (no silent cast)")
    if ids.ndim != 1:
        raise ValueError(f"{name} must have shape (m,), not {ids.shape}")
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    bad = (ids < 0) | (ids >= n)
    if bad.any():
        raise ValueError(f"{name} must lie in [0, {n}): {int(bad.sum())} of {len(ids)} do not (the first: {int(ids[bad][0])})")
    return ids


def host_float64(a, name, shapes=None, numbers_only=False):
    """Values on the host (an array or a list) as contiguous float64, of one of `shapes` (None: the caller checks the shape).  A float
    dtype other than float64 is a TypeError (no silent cast); integers and bools convert.
    numbers_only, as found: update_neumann_flags refuses every other kind (complex, strings, objects) with the TypeError; update_points
    and update_permeability leave them to numpy's conversion -- a complex K is taken with a ComplexWarning, its imaginary part dropped."""
    try:
        a = np.asarray(a)
        if (a.dtype.kind == "f" and a.dtype != np.float64) or (numbers_only and a.dtype.kind not in "fiub"):
            raise TypeError(f"{name} must be float64{', integers or bool' if numbers_only else ''}, not {a.dtype} (no silent cast)")
        a = np.ascontiguousarray(a, dtype=np.float64)
    except ValueError as e:
        raise ValueError(f"{name} cannot be converted to float64: {e}") from e
    if shapes is not None:
        check_shape(a.shape, name, shapes)
    return a


def require_device_tensor(t, name, device, beside, cpu_tensor_passes=False):
    """`t` must be a torch tensor on a GPU (cuda:`device`, says the message) because the argument `beside` is one (TypeError: host and
    device arguments cannot be mixed).
    cpu_tensor_passes, as found: the whole-table update_permeability lets a CPU tensor through to the device check, which then raises
    ValueError ("must be on cuda:0, not cpu"); every other path raises the TypeError here."""
    import torch
    if not isinstance(t, torch.Tensor) or not (t.is_cuda or cpu_tensor_passes):
        raise TypeError(f"{name} must be a torch.Tensor on cuda:{device} when {beside} is, not " +
                        (f"one on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__))


def device_tensor(t, name, device, beside, shapes=None, also=(), cpu_tensor_passes=False):
    """A float64 torch tensor -- or one of a dtype named in `also` -- on cuda:`device`, of one of `shapes` (None: the caller checks
    the shape), detached and contiguous."""
    import torch
    require_device_tensor(t, name, device, beside, cpu_tensor_passes)
    if t.dtype != torch.float64 and str(t.dtype).split(".")[-1] not in also:
        raise TypeError(f"{name} must be {_one_of(('float64',) + also)}, not {t.dtype} (no silent cast)")
    if not t.is_cuda or t.get_device() != device:
        raise ValueError(f"{name} must be on cuda:{device}, not {t.device}")
    if shapes is not None:
        check_shape(t.shape, name, shapes)
    return t.detach().contiguous()


def device_ids(t, name, device):
    """Ids in a torch tensor on a GPU: int32 or int64, on cuda:`device`, 1-D.  Returns how many; membership in [0, n) is checked on the device,
    by the kernel that reads them."""
    import torch
    if t.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"{name} must be int32 or int64, not {t.dtype} (no silent cast)")
    if not t.is_cuda or t.get_device() != device:
        raise ValueError(f"{name} must be on cuda:{device}, not {t.device}")
    if t.dim() != 1:
        raise ValueError(f"{name} must have shape (m,), not {tuple(t.shape)}")
    return int(t.shape[0])
