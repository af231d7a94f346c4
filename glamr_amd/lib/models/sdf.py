"""Multi-person penetration loss on MI355X -- stands in for `SDFLoss` of the third-party `sdf` package that the reference imports
(global_recon_model.py:18,65: `SDFLoss(self.smpl.faces, robustifier=True)`; loss_func.py:274-290).

Same class name and call:

    sdf_loss = SDFLoss(faces, grid_size=32, robustifier=True)
    loss = sdf_loss(vertices (N, V, 3), translation=None, scale_factor=0.2)       # -> scalar: one frame, N persons
    per_frame = sdf_loss.frames(vertices (F, P, V, 3), active (F, P))             # -> (F,): a batch of frames

The package is neither part of the reference nor installable here, so the term is RESTATED from the published algorithm; the definition is
DESIGN.md 18 and is unpinned against the package.  Boxes, overlap flags, the signed-distance grids, the sampling, the robustifier and the
gradient to the sampled vertices run in HIP kernels behind `glamr_sdf_penetration` (include/glamr_hip.h); this file owns the face table and
gives the call autograd semantics.  There is no CPU implementation: tensors must live on a HIP device.  `faces` must describe a closed mesh
oriented outwards (SMPL's is).
"""
import numpy as np
import torch
from torch import nn

from ... import _lib


class _PenetrationFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, module, verts, active, scale_factor):
        F_, P, V = verts.shape[:3]
        dev = verts.device
        faces = module._faces_on(dev)
        L = _lib.lib()
        loss = torch.empty((F_,), device=dev, dtype=torch.float32)
        want_grad = verts.requires_grad
        g = torch.empty_like(verts) if want_grad else None
        if F_ > 0:
            nbytes = L.glamr_sdf_workspace_bytes(F_, P, V, faces.shape[0], module.grid_size)
            if nbytes == 0:
                raise ValueError('SDFLoss: sizes out of range (frames %d, persons %d (1..32), vertices %d, faces %d, grid %d (2..64))'
                                 % (F_, P, V, faces.shape[0], module.grid_size))
            ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
            _lib.check(L.glamr_sdf_penetration(_lib.ptr(verts), _lib.ptr(active), _lib.ptr(faces), F_, P, V, faces.shape[0], module.grid_size,
                                               float(scale_factor), module.rho, _lib.ptr(loss), _lib.ptr(g), None, None, None, _lib.ptr(ws),
                                               _lib.current_stream()))
        ctx.save_for_backward(g)
        return loss

    @staticmethod
    def backward(ctx, g_loss):
        g, = ctx.saved_tensors
        if g is None:
            return None, None, None, None
        return None, g * g_loss.reshape(-1, 1, 1, 1), None, None


class SDFLoss(nn.Module):

    def __init__(self, faces, grid_size=32, robustifier=None, debugging=False):
        super().__init__()
        faces = np.ascontiguousarray(np.asarray(faces.detach().cpu() if torch.is_tensor(faces) else faces).astype(np.int32))
        if faces.ndim != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
            raise ValueError('SDFLoss: faces must be (NF, 3), got %s' % (faces.shape,))
        if not 2 <= int(grid_size) <= 64:
            raise ValueError('SDFLoss: grid_size must lie in 2..64, got %r' % (grid_size,))
        self.register_buffer('faces', torch.from_numpy(faces), persistent=False)
        self.grid_size = int(grid_size)
        self.robustifier = robustifier
        self.rho = float(robustifier) if robustifier else 0.0          # robustifier=True: rho = 1 (global_recon_model.py:65)
        self._dev_faces = {}

    def _faces_on(self, dev):
        key = (dev.type, dev.index)
        if key not in self._dev_faces:
            self._dev_faces[key] = self.faces.to(dev).contiguous()
        return self._dev_faces[key]

    def frames(self, vertices, active=None, scale_factor=0.2):
        """vertices (F, P, V, 3) fp32 on the HIP device, active (F, P) bool / uint8 or None (everybody) -> the term per frame (F,);
        differentiable with respect to `vertices`.  Vertices of inactive persons are never read."""
        if not (torch.is_tensor(vertices) and vertices.is_cuda):
            raise RuntimeError('SDFLoss runs on the HIP device only (there is no CPU implementation); vertices live on %s'
                               % (vertices.device if torch.is_tensor(vertices) else type(vertices).__name__))
        if vertices.dim() != 4 or vertices.shape[-1] != 3:
            raise ValueError('SDFLoss.frames: vertices must be (F, P, V, 3), got %s' % (tuple(vertices.shape),))
        verts = vertices.float().contiguous()
        if active is None:
            act = torch.ones(verts.shape[:2], device=verts.device, dtype=torch.uint8)
        else:
            if tuple(active.shape) != tuple(verts.shape[:2]):
                raise ValueError('SDFLoss.frames: active must be (F, P) = %s, got %s' % (tuple(verts.shape[:2]), tuple(active.shape)))
            act = active.to(device=verts.device, dtype=torch.uint8).contiguous()
        return _PenetrationFn.apply(self, verts, act, scale_factor)

    def forward(self, vertices, translation=None, scale_factor=0.2):
        """One frame: vertices (N, V, 3) of N persons (+ translation, broadcast, when given) -> scalar."""
        if translation is not None:
            vertices = vertices + translation.reshape(vertices.shape[0], -1, 3)
        return self.frames(vertices[None], None, scale_factor)[0]
