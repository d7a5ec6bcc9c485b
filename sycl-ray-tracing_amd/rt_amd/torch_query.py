"""Ray queries on torch tensors: rt_query_device on the tensor's memory and on torch's
current stream, no host copies.

    from rt_amd import torch_query
    hits = torch_query.query(rk, rays)               # int32 [n, 11]
    t = hits.view(torch.float32)[:, 2]               # the float words: t, point, normal
    seen = torch_query.query(rk, rays, mode="any")   # int32 [n]

torch is imported here only, never when the package is imported.
"""
from __future__ import annotations


def query(rk, rays, mode: str = "closest", exact: bool = False):
    """rk: a RenderKernel on the product library. rays: a contiguous float32 [n, 6] tensor
    (origin, direction) on the context's (root) device. Runs on torch.cuda.current_stream()
    of that device and returns without waiting, like any torch operation. mode "closest":
    an int32 [n, 11] tensor, rt_intersect's record ({found, primitive, t, point[3],
    normal[3], u, v}; .view(torch.float32) gives the float words); "any": int32 [n], 1 where
    there is a hit. exact=True: every query takes the exact walk (RT_QUERY_EXACT)."""
    import torch

    if not isinstance(rays, torch.Tensor) or not rays.is_cuda:
        raise TypeError("rays must be a tensor on the GPU")
    if rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] != 6 or not rays.is_contiguous():
        raise ValueError("rays must be a contiguous float32 [n, 6] tensor")
    n = int(rays.shape[0])
    out = torch.empty((n, 11) if mode == "closest" else (n,), dtype=torch.int32, device=rays.device)
    stream = torch.cuda.current_stream(rays.device)
    rk.query_device(rays.data_ptr(), n, out.data_ptr(), mode=mode, exact=exact, stream=stream.cuda_stream)
    return out
