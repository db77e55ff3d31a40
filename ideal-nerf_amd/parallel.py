"""Multi-GPU tiling of the per-ray path: one process per GPU, weights replicated, the
frame split into contiguous row bands, one all-gather of the rendered tiles per frame -- or,
for a whole clip, whole frames dealt round-robin to the ranks (``frames_of``) and assembled in
order on rank 0 (``ClipAssembler``): no collective until a frame is finished bytes.

This replaces the reference's single-process ``nn.DataParallel`` ray scatter / output
gather (NeRFs/HeadNeRF/train/distribute_nerf.py:457-466, test/test_distribute_nerf.py:
378-387): rays are independent, so each rank derives its own rays from (row0, nrows, c2w)
-- no input scatter -- and only the outputs are exchanged (393 KB per rank for a 512^2
frame at 8 ranks; one RCCL all_gather over xGMI, latency-bound).
"""
from typing import List, Optional, Tuple

import torch
import torch.distributed as dist


def row_band(H: int, rank: int, world: int) -> Tuple[int, int]:
    """Rows [r0, r1) of an H-row frame owned by ``rank``: bands differ by at most one row
    and tile the frame exactly."""
    base, rem = divmod(H, world)
    r0 = rank * base + min(rank, rem)
    return r0, r0 + base + (1 if rank < rem else 0)


def all_bands(H: int, world: int) -> List[Tuple[int, int]]:
    return [row_band(H, r, world) for r in range(world)]


def gather_rows(tile: torch.Tensor, H: int, group=None, force: bool = False) -> torch.Tensor:
    """tile: this rank's [rows_r, W, C] band -> the full [H, W, C] frame on every rank.
    Bands may differ by one row, so tiles are padded to the widest band for the
    fixed-size all_gather and trimmed afterwards.  ``force``: issue the collective even on a
    one-rank communicator (how a one-GPU box exercises the RCCL call itself)."""
    if not (dist.is_available() and dist.is_initialized()) or (dist.get_world_size(group) == 1 and not force):
        return tile
    world = dist.get_world_size(group)
    bands = all_bands(H, world)
    max_rows = max(b - a for a, b in bands)
    pad = tile
    if tile.shape[0] < max_rows:
        pad = torch.cat([tile, tile.new_zeros((max_rows - tile.shape[0],) + tuple(tile.shape[1:]))], 0)
    out = tile.new_empty((world * max_rows,) + tuple(tile.shape[1:]))
    dist.all_gather_into_tensor(out, pad.contiguous(), group=group)
    if world * max_rows == H:     # equal bands (512 rows over 8 ranks): the gathered buffer IS the frame, no copy
        return out
    parts = [out[r * max_rows: r * max_rows + (b - a)] for r, (a, b) in enumerate(bands)]
    return torch.cat(parts, 0)


def average_gradients(params, group=None) -> None:
    """Data-parallel training (beyond the reference's DataParallel): every rank renders its
    own ray batch and the gradients are averaged before the optimizer step.  Both FaceNeRFs, the audio
    nets and the latent codes are 5.8 MB of gradients: they are flattened into ONE bucket and reduced
    with a single all-reduce (xGMI rings are latency-bound at this size; per-tensor calls would pay
    that latency ~60 times), then scattered back in place.  Parameters without a gradient on this
    rank contribute zeros, so ranks may differ in which optional branches they touched."""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return
    params = [p for p in params if p.requires_grad]
    if not params:
        return
    world = dist.get_world_size(group)
    flat = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1).to(torch.float32) for p in params])
    dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
    flat.div_(world)
    off = 0
    for p in params:
        n = p.numel()
        g = flat[off:off + n].view_as(p).to(p.dtype)
        if p.grad is None:
            p.grad = g.clone()
        else:
            p.grad.copy_(g)
        off += n


def frames_of(rank: int, world: int, n_frames: int) -> range:
    """Frame-parallel clip rendering: rank r renders frames r, r + N, r + 2N, ...  Shares are
    disjoint, increasing, cover the clip and differ by at most one frame."""
    if not 0 <= rank < world:
        raise ValueError(f"rank {rank} outside a world of {world}")
    return range(rank, max(int(n_frames), 0), world)


class ClipAssembler:
    """Puts the frames of ``frames_of`` shares back in clip order in front of one writer.

    Every rank calls ``push(u8_frame, nonfinite)`` once per round, in its ``frames_of`` order; a rank whose share
    is one frame short calls ``push(None)`` in the last round.  Round k carries the frames k*N .. k*N+N-1 to
    rank 0 in one ``dist.gather`` of equal uint8 payloads (the frame's bytes and one flag byte: host tensors
    under gloo, device tensors under RCCL); rank 0 hands them to ``sink.submit_u8`` in frame order and drops the
    placeholders.  Each rank has converted its own frame, so only bytes travel.  ``sink`` is anything with
    ``submit_u8(frame, nonfinite)`` and ``release()`` (``frame_io.FrameSink``); ranks other than 0 pass None.
    Without an initialised process group, or with one rank, push() is sink.submit_u8()."""

    def __init__(self, sink, n_frames: int, group=None):
        self.sink, self.n_frames, self.group = sink, int(n_frames), group
        self.on = dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1
        self.world = dist.get_world_size(group) if self.on else 1
        self.rank = dist.get_rank(group) if self.on else 0
        self.root = dist.get_global_rank(group, 0) if self.on and group is not None else 0
        self.device_payloads = self.on and dist.get_backend(group) == "nccl"
        self.rounds = -(-self.n_frames // self.world)
        self.round = 0
        self.shape: Optional[Tuple[int, ...]] = None
        self._flagged: List[int] = []     # frames whose flag reached this object as a host bool
        if self.rank == 0 and sink is None:
            raise ValueError("rank 0 assembles the clip: it needs a sink")

    def _agree_on_shape(self, frame) -> None:
        """Round 0: rank 0 (which holds frame 0) tells the frame shape to ranks that may never hold one."""
        dev = torch.device("cuda", torch.cuda.current_device()) if self.device_payloads else torch.device("cpu")
        hw = torch.tensor(list(frame.shape) if self.rank == 0 else [0, 0, 0], dtype=torch.int64, device=dev)
        dist.broadcast(hw, src=self.root, group=self.group)
        self.shape = tuple(int(v) for v in hw.tolist())
        self.payload_device = dev

    def push(self, frame, nonfinite=False) -> None:
        """frame: uint8 [H, W, 3] (device or host tensor, or ndarray), or None for the placeholder of an uneven last
        round; nonfinite: bool, or the int32 device flag the frame's conversion set."""
        if self.round >= self.rounds:
            raise RuntimeError(f"push() number {self.round + 1} for a clip of {self.rounds} round(s)")
        index = self.round * self.world + self.rank
        if (frame is None) != (index >= self.n_frames):
            raise ValueError(f"round {self.round}: rank {self.rank} " + ("has no frame left" if frame is not None else f"owes frame {index}"))
        if not self.on:
            if not isinstance(nonfinite, torch.Tensor) and nonfinite:
                self._flagged.append(index)
            self.sink.submit_u8(frame, nonfinite)
            self.round += 1
            return
        if frame is not None and not isinstance(frame, torch.Tensor):
            frame = torch.as_tensor(frame)
        if self.shape is None:
            self._agree_on_shape(frame)
        n = self.shape[0] * self.shape[1] * self.shape[2]
        payload = torch.zeros(n + 1, dtype=torch.uint8, device=self.payload_device)
        if frame is not None:
            if frame.dtype != torch.uint8 or tuple(frame.shape) != self.shape:
                raise ValueError(f"expected uint8 {list(self.shape)}, got {frame.dtype} {list(frame.shape)}")
            flag = (nonfinite.reshape(-1)[:1] != 0) if isinstance(nonfinite, torch.Tensor) else torch.tensor([bool(nonfinite)])
            payload[:n] = frame.reshape(-1).to(self.payload_device)
            payload[n:] = flag.to(device=self.payload_device, dtype=torch.uint8)
        parts = [torch.empty_like(payload) for _ in range(self.world)] if self.rank == 0 else None
        dist.gather(payload, parts, dst=self.root, group=self.group)
        if self.rank == 0:
            for r, part in enumerate(parts):
                if self.round * self.world + r >= self.n_frames:
                    break       # placeholders of the uneven last round
                flag = part[n:].to(torch.int32) if part.is_cuda else bool(part[n])
                if flag is True:
                    self._flagged.append(self.round * self.world + r)
                self.sink.submit_u8(part[:n].view(self.shape), flag)
        self.round += 1

    def close(self):
        """After the last round: rank 0 releases the sink and returns dict(n_frames, nonfinite_frames); others None."""
        if self.round != self.rounds:
            raise RuntimeError(f"close() after {self.round} of {self.rounds} round(s)")
        if self.rank != 0:
            return None
        self.sink.release()
        # a device flag is read by the sink together with the frame's bytes: the sink knows those frames
        flagged = set(self._flagged) | {int(i) for i in getattr(self.sink, "nonfinite_frames", ())}
        return dict(n_frames=self.n_frames, nonfinite_frames=sorted(flagged))


def gather_frame_rows(rows: torch.Tensor, n_frames: int, group=None) -> Optional[torch.Tensor]:
    """The per-frame result rows of a frame-parallel loop back in frame order: every rank passes its
    ``[len(frames_of(rank, world, n_frames)), ...]`` tensor (row k belongs to frame ``k * world + rank``) and rank 0 receives
    ``[n_frames, ...]``, the other ranks None.  ONE ``dist.gather`` of equal payloads (a rank whose share is a frame short pads
    a zero row, dropped again on rank 0): host tensors under gloo (a device tensor is copied to the host first -- these are
    score rows, not frames), device tensors under RCCL.  Without an initialised process group, or with one rank, ``rows`` is
    returned as it is."""
    n_frames = int(n_frames)
    on = dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1
    rank, world = (dist.get_rank(group), dist.get_world_size(group)) if on else (0, 1)
    mine = len(frames_of(rank, world, n_frames))
    if rows.shape[0] != mine:
        raise ValueError(f"rank {rank} of {world} holds {mine} of {n_frames} frames, got {rows.shape[0]} rows")
    if not on:
        return rows
    device = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend(group) == "nccl" else torch.device("cpu")
    rounds = -(-n_frames // world)
    payload = torch.zeros((rounds,) + tuple(rows.shape[1:]), dtype=rows.dtype, device=device)
    payload[:mine] = rows.to(device)
    parts = [torch.empty_like(payload) for _ in range(world)] if rank == 0 else None
    dist.gather(payload, parts, dst=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
    if rank != 0:
        return None
    return torch.stack(parts, 1).reshape((rounds * world,) + tuple(rows.shape[1:]))[:n_frames]
