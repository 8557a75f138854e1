"""A regular grid of irradiance probes for DeviceScene.probe_lookup (rayca_hip_probe_lookup_device): where the probes stand, and how
to bake them with DeviceScene.gather.  The grid is three plain triples; nothing in the lookup's specification depends on how the
probes' coefficients were made."""
import numpy as np

from .ambient import sphere_directions


class ProbeGrid:
    """origin: the centre of probe (0, 0, 0); cell: the spacing per axis (> 0); dims: (nx, ny, nz), each >= 1.  Probe (ix, iy, iz)
    has index (iz * ny + iy) * nx + ix and centre origin + float(i) * cell per axis."""

    def __init__(self, origin, cell, dims):
        self.origin = np.asarray(origin, np.float32).reshape(3)
        self.cell = np.asarray(cell, np.float32).reshape(3)
        self.dims = tuple(int(d) for d in dims)
        if len(self.dims) != 3 or min(self.dims) < 1 or self.dims[0] * self.dims[1] * self.dims[2] > 1 << 24:
            raise ValueError(f"dims: {dims}, expected three counts >= 1 with a product of at most 2**24")
        if not (np.isfinite(self.origin).all() and np.isfinite(self.cell).all() and (self.cell > 0).all()):
            raise ValueError("origin and cell: finite values, cell > 0")

    @classmethod
    def around(cls, lo, hi, dims, margin=0.0):
        """The grid whose outermost probes stand `margin` (world units; negative: inside) outside the box lo..hi.  An axis with
        one probe puts it at the middle of the box and gets a cell of 1."""
        lo, hi = np.asarray(lo, np.float64).reshape(3) - margin, np.asarray(hi, np.float64).reshape(3) + margin
        d = np.array([int(x) for x in dims])
        cell = np.where(d > 1, (hi - lo) / np.maximum(d - 1, 1), 1.0)
        origin = np.where(d > 1, lo, 0.5 * (lo + hi))
        return cls(origin, cell, dims)

    @property
    def count(self):
        return self.dims[0] * self.dims[1] * self.dims[2]

    def positions(self) -> np.ndarray:
        """(M, 3) float32 probe centres in index order, by the specification's own two operations: float(i) * cell, + origin,
        each rounded to f32."""
        nx, ny, nz = self.dims
        iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        i = np.stack([ix, iy, iz], -1).reshape(-1, 3).astype(np.float32)
        step = (i * self.cell).astype(np.float32)
        return (self.origin + step).astype(np.float32)

    def bake(self, ds, config, samples=64, sample=0, *, stream=None, context=0, direct=False):
        """(sh (M, 9, 4) float32, kept (M,) int32) on ds's device: DeviceScene.gather at the probes' centres with the normal
        (0, 0, 1), sphere_directions(samples) and weights of 4 pi -- the projections of the incoming radiance onto the nine basis
        functions, which the lookup takes as they are.  A probe none of whose samples is finite has kept 0.
        direct: add the light that reaches the centres straight from the scene's lights -- DeviceScene.direct without normals,
        its "sh", in the same units -- which no gather ray can find for a point light: sh = gather's sh + direct's sh, one
        torch addition on the same stream.  kept stays gather's."""
        import torch
        dev = torch.device("cuda", ds.device)
        p = torch.from_numpy(self.positions()).to(dev)
        n = torch.zeros_like(p)
        n[:, 2] = 1.0
        dirs = torch.from_numpy(sphere_directions(samples)).to(dev)
        weights = torch.full((samples,), float(np.float32(4.0 * np.pi)), dtype=torch.float32, device=dev)
        r = ds.gather(p, n, config, samples=samples, dirs=dirs, weights=weights, sample=sample, outputs=("sh", "kept"), stream=stream, context=context)
        if not direct:
            return r["sh"], r["kept"]
        d = ds.direct(p, None, config, sample=sample, want=("sh",), stream=stream, context=context)
        with torch.cuda.stream(ds.torch_stream(stream)):
            return r["sh"] + d["sh"], r["kept"]
