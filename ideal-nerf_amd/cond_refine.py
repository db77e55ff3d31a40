"""Joint refinement of two more inputs of the offline pipeline during training: the per-frame expression rows and the
background image (the reference has no counterpart: both are ordinary tensors of its torch graph, but nothing there trains
them).

The expression rows of ``transforms_exp_*.json`` come from the face tracker whose camera jitter ``pose_refine`` corrects,
frame by frame; ``bc.jpg`` is a heuristic composite whose ghosting is burnt into every training target -- it is the colour of
each ray's last sample.  ``ExprRefiner`` holds one additive correction per training frame, ``Background`` the image itself as
a parameter.  The gradients reach them through the render: ``autograd.RenderRaysFn`` returns d expr (the conditioning fold of
both passes, ``idealnerf_pass_bwd_ex``) and d bc (``g_rgb_map * last_weight`` of each pass: rgb_map is linear in the
background) when, and only when, those inputs require one.
"""
import torch


class ExprRefiner(torch.nn.Module):
    """``deltas[n_frames, dim_expr]`` per training frame, zero at the start (the tracker's expressions)."""

    def __init__(self, n_frames: int, dim_expr: int):
        super().__init__()
        self.deltas = torch.nn.Parameter(torch.zeros(int(n_frames), int(dim_expr), dtype=torch.float32))

    def forward(self, index: int, expr: torch.Tensor) -> torch.Tensor:
        """expr [..., dim_expr] of frame ``index``, as either loader returns it -> ``expr + deltas[index]`` of the same shape, on
        the deltas' device, with the graph edge to that row alone."""
        return expr.to(device=self.deltas.device, dtype=self.deltas.dtype) + self.deltas[int(index)]


class Background(torch.nn.Module):
    """The background as a parameter: ``image`` float32 [H, W, 3], initialised from the dataset's background (uint8 [H, W, 3])
    as ``uint8 / 255`` -- evaluated in float64 and rounded to float32, bit for bit the values both loaders hand the renderer
    (``GetData.background_img`` after ``Network.forward``'s cast, ``ops.byte_tables``) --, so the first step renders over
    exactly what a run without the option renders over.

    The values are NOT clamped to [0, 1] while they train: the render is linear in them and the loss pulls them towards the
    targets, which lie inside; ``to8b`` clips at the very end, where an image is written."""

    def __init__(self, image: torch.Tensor):
        super().__init__()
        if image.dim() != 3 or image.shape[-1] != 3:
            raise ValueError(f"the background must be [H, W, 3], got {list(image.shape)}")
        if image.dtype == torch.uint8:
            start = (image.detach().to(torch.float64) / 255.0).to(torch.float32)
        else:
            start = image.detach().to(torch.float32).clone()
        self.image = torch.nn.Parameter(start)

    def rows(self, sel: torch.Tensor) -> torch.Tensor:
        """The pixels of a batch by flat index (``sel`` int64 [n], row-major over H x W) -> [n, 3].  An index that occurs more than
        once gets the sum of its rows' gradients (the gather's backward adds)."""
        return self.image.reshape(-1, 3)[sel]

    def forward(self) -> torch.Tensor:
        """The whole image [H, W, 3], for a full-frame render."""
        return self.image
