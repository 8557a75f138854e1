"""Tensors that are not contiguous, for the tests of the wrappers that copy such inputs."""


def strided(x):
    """The values of `x` -- a torch tensor of two or more dimensions, or a dict of such, nested or not; anything else comes back as
    it is -- in tensors that are not contiguous: views into tensors one column wider."""
    import torch
    if isinstance(x, dict):
        return {k: strided(v) for k, v in x.items()}
    if not isinstance(x, torch.Tensor):
        return x
    wide = torch.empty((x.shape[0], x.shape[1] + 1) + tuple(x.shape[2:]), dtype=x.dtype, device=x.device)
    view = wide[:, :x.shape[1]]
    view.copy_(x)
    assert x.shape[0] > 1 and not view.is_contiguous()
    return view
