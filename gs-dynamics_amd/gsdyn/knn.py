"""Exact k-nearest-neighbour search: the neighbour lists of the rigidity losses and the outlier filter.

Definition, for fp32 points [N, 3]: the distance of query i to point j is ``d2 = (dx*dx + dy*dy) + dz*dz`` with ``dx = p[i].x - p[j].x``
and so on, every operation in the tensor's dtype, in that order, unfused.  Row i holds the k smallest under the total order (d2
ascending, then j ascending), written in that order.  With ``exclude_self`` the point j = i is left out by identity: a duplicate of
point i with a lower index is a legitimate first neighbour.  The order is total, so there is one right answer."""
import torch

KERNEL_MAX_K = 64     # csrc/gsr_knn.hip keeps the running best-k one entry per lane of a wave


def _knn_torch(points: torch.Tensor, k: int, exclude_self: bool):
    """The definition in plain torch: chunked rows, direct differences, a stable sort for the index tie-break (no topk: its tie order
    is unspecified)."""
    N = points.shape[0]
    dev = points.device
    rows = max(1, min(N, (1 << 22) // N))
    take = k + 1 if exclude_self else k
    cols = torch.arange(k, device=dev)[None]
    idx_out, d2_out = [], []
    x, y, z = points[:, 0], points[:, 1], points[:, 2]
    for s in range(0, N, rows):
        q = points[s:s + rows]
        dx, dy, dz = q[:, 0, None] - x[None], q[:, 1, None] - y[None], q[:, 2, None] - z[None]
        d2 = (dx * dx + dy * dy) + dz * dz
        ds, order = torch.sort(d2, dim=1, stable=True)
        ds, order = ds[:, :take], order[:, :take]
        if exclude_self:
            me = torch.arange(s, s + q.shape[0], device=dev)[:, None]
            is_me = order == me
            # where the query sits among its first k + 1 (k + 1: not among them); the columns from there on move up by one
            pos = torch.where(is_me.any(1), is_me.int().argmax(1), torch.full((q.shape[0],), take, device=dev))[:, None]
            pick = cols + (cols >= pos).long()
            ds, order = ds.gather(1, pick), order.gather(1, pick)
        idx_out.append(order)
        d2_out.append(ds)
    return torch.cat(idx_out).contiguous(), torch.cat(d2_out).contiguous()


def knn_points(points: torch.Tensor, k: int, *, exclude_self: bool = False):
    """The k nearest points of every point: ``(idx [N, k] int64, d2 [N, k])`` by the definition of this module.

    A contiguous fp32 [N, 3] tensor on a HIP device with k <= 64 takes the kernels (csrc/gsr_knn.hip: a uniform grid built on the device,
    one wave per query, no host read-back); every other input -- CPU, fp64, a larger k, a strided view -- takes the plain-torch
    statement of the same definition in the tensor's dtype, so both give the same indices and, in fp32, the same bits.
    Rows that involve non-finite coordinates are unspecified."""
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("knn_points: points must be [N, 3]")
    N, k = int(points.shape[0]), int(k)
    if k < 1 or k > N - (1 if exclude_self else 0):
        raise ValueError(f"knn_points: need 1 <= k <= N - (1 if exclude_self else 0); got N = {N}, k = {k}, exclude_self = {bool(exclude_self)}")
    if points.is_cuda and points.dtype == torch.float32 and points.is_contiguous() and k <= KERNEL_MAX_K:
        from diff_gaussian_rasterization import _hip
        return _hip.knn(points, k, exclude_self=bool(exclude_self))
    with torch.no_grad():
        return _knn_torch(points.detach(), k, bool(exclude_self))
