"""Device-resident training set and size-bucketed ragged batches.

The reference builds every batch on the host: joblib-cached samples, `pad_batch_inputs` / `pad_batch_transcripts` in the collate
function (src/data/preprocessing.py:55-144), one H2D copy of the padded plane per step.  Here the whole set lives in HBM -- score
images as the uint8 grays they are before their `/ 255`, spectrograms as fp32 -- packed back to back in ONE buffer, and a batch is a
list of sample indices plus one launch of `omr_gather_ragged_batch` (csrc/batch_gather.hip) that writes the zero-padded plane in the
compute dtype.  What comes out is, to the bit, what `image.collate_ragged` / `collate_ragged_pairs` build from the same samples:
the `(x, sizes)` pairs of the ragged route of `Transformer.training_step` and `MultimodalTransformer.training_step`.

  ResidentStore      the packed buffer of one modality: append / freeze / gather
  ResidentDataset    one or two stores plus the host token lists: batch(indices, dtype, records=None), eval_batches()
  plan_batches       which samples share a batch: shuffle, sort chunks by size, cut under a padded-pixel / padded-token budget
  shard_batches      the plan's batches of one rank; padded_ratio: real / padded pixels of a plan
  ResidentLoader     the training loader over a ResidentDataset (set_epoch / __len__ / __iter__: what lightning_shim.Trainer.fit uses)

The plan is host arithmetic on the size table only (no torch.cuda); the stores run on the GPU only (HIP kernel, no CPU fallback)."""
from __future__ import annotations

from typing import Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import augment, kernels

Tensor = torch.Tensor

KINDS = {"u8": torch.uint8, "f32": torch.float32}


# ------------------------------------------------------------------------------------------------ the packed store

class ResidentStore:
    """Samples [h, w] of different sizes back to back in one device buffer.  kind "u8": floats that are k / 255 (every output of
    `image.preprocess_image`), kept as the byte k -- `append` REFUSES a tensor the bytes do not reproduce to the bit, so the store
    is lossless or raises; kind "f32": any fp32 values (spectrograms), copied.  The buffer grows geometrically (it never holds more
    than twice what is in it, `reserve` sizes it once when the total is known); a sample is a slice of it, never a tensor of its own.
    The host keeps the sizes and offsets; their device copies are made once, by `freeze()` or the first `gather`."""

    def __init__(self, kind: str, device=None):
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {sorted(KINDS)}, got {kind!r}")
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("ResidentStore lives on the GPU (HIP kernel); there is no CPU fallback")
        self.kind, self.device, self.store_dtype = kind, device, KINDS[kind]
        self.buf = torch.empty((0,), dtype=self.store_dtype, device=device)
        self.used = 0                                   # elements of buf in use
        self._hw: List[Tuple[int, int]] = []
        self._offsets: List[int] = []
        self._sizes_host: Optional[Tensor] = None       # int64 [N, 2], rebuilt after an append
        self._tables = None                             # (offsets int64 [N], sizes int32 [N, 2]) on the device
        # a one-sample table for append's own read-back: offset 0 of the slice, index 0; only the size changes
        self._one_off = torch.zeros((1,), dtype=torch.int64, device=device)
        self._one_idx = torch.zeros((1,), dtype=torch.int32, device=device)

    def __len__(self) -> int:
        return len(self._hw)

    @property
    def sizes(self) -> Tensor:
        """int64 [N, 2] = (h_n, w_n) on the host."""
        if self._sizes_host is None:
            self._sizes_host = torch.tensor(self._hw, dtype=torch.int64).reshape(-1, 2)
        return self._sizes_host

    def reserve(self, elements: int) -> None:
        """Make room for `elements` elements in all (one allocation instead of the doublings)."""
        if elements > self.buf.numel():
            new = torch.empty((elements,), dtype=self.store_dtype, device=self.device)
            new[:self.used] = self.buf[:self.used]
            self.buf = new

    def append(self, x: Tensor) -> int:
        """x: float [h, w] or [1, h, w], host or device.  Returns the sample's index."""
        if x.dim() == 3 and x.shape[0] == 1:
            x = x[0]
        if x.dim() != 2 or x.numel() == 0 or not x.is_floating_point():
            raise ValueError(f"expected a float sample [h, w] or [1, h, w], got {x.dtype} {tuple(x.shape)}")
        h, w = int(x.shape[0]), int(x.shape[1])
        n = h * w
        if self.used + n > self.buf.numel():
            self.reserve(max(self.used + n, 2 * self.buf.numel()))
        x = x.to(self.device, torch.float32).contiguous()
        dst = self.buf[self.used:self.used + n]
        if self.kind == "u8":
            dst.copy_((x * 255.0).round().clamp_(0.0, 255.0).view(-1))          # a NaN or a value off [0, 1] fails the read-back below
            size = torch.tensor([[h, w]], dtype=torch.int32).to(self.device)
            back = kernels.gather_ragged_batch(dst, self._one_off, size, self._one_idx, h, w, torch.float32)
            if not torch.equal(back.view(torch.int32).view(h, w), x.view(torch.int32)):
                bad = int((back.view(torch.int32).view(h, w) != x.view(torch.int32)).sum())
                raise ValueError(f"ResidentStore('u8'): {bad} of {n} values of sample {len(self)} are not k / 255 in fp32; the store is lossless "
                                 "or it refuses -- keep such data in a store of kind 'f32'")
        else:
            dst.copy_(x.view(-1))
        self._hw.append((h, w))
        self._offsets.append(self.used)
        self.used += n
        self._sizes_host = self._tables = None
        return len(self._hw) - 1

    def freeze(self) -> "ResidentStore":
        """Upload the offset and size tables (a later `append` drops them again)."""
        if self._tables is None:
            if not self._hw:
                raise ValueError("the store is empty")
            off = torch.tensor(self._offsets, dtype=torch.int64).to(self.device)
            self._tables = (off, self.sizes.to(torch.int32).to(self.device))
        return self

    def gather(self, indices: Sequence[int], dtype: torch.dtype, pad_value: float = 0.0, records=None) -> Tuple[Tensor, Tensor]:
        """-> (x [B, 1, Hmax, Wmax] in `dtype` on the device: sample indices[b] in the top-left corner of plane b, pad_value elsewhere;
        sizes int64 [B, 2] on the host): `image.collate_ragged` of those samples (pad 0).  The plane is the maximum over the batch,
        taken from the host table: no device read-back; the index list goes up non-blocking from pinned memory.

        records: `augment.AUG_DTYPE` [B], one per index -- the batch is built by `omr_gather_augmented_batch` instead: row b is sample
        indices[b] under record b, the plane is the maximum of the records' extents and `sizes` ARE those extents (what the ragged
        route has to be told).  The records go up like the index list."""
        idx = torch.as_tensor(indices, dtype=torch.int64).reshape(-1)
        if idx.numel() == 0:
            raise ValueError("gather needs at least one index")
        if int(idx.min()) < 0 or int(idx.max()) >= len(self):
            raise IndexError(f"sample index out of range [0, {len(self)})")
        off, sizes_dev = self.freeze()._tables
        idx_dev = idx.to(torch.int32).pin_memory().to(self.device, non_blocking=True)
        if records is None:
            sizes = self.sizes[idx]
            H, W = int(sizes[:, 0].max()), int(sizes[:, 1].max())
            x = kernels.gather_ragged_batch(self.buf, off, sizes_dev, idx_dev, H, W, dtype, pad_value)
            return x, sizes
        records = np.ascontiguousarray(np.asarray(records).reshape(-1))
        if records.dtype != augment.AUG_DTYPE or records.shape[0] != idx.numel():
            raise ValueError(f"records must be augment.AUG_DTYPE [{idx.numel()}], got {records.dtype} {records.shape}")
        sizes = torch.from_numpy(augment.extents(records))
        if int(sizes.min()) < 1:
            raise ValueError("a record's extent (out_h, out_w) must be at least 1 x 1")
        H, W = int(sizes[:, 0].max()), int(sizes[:, 1].max())
        raw = torch.from_numpy(records.view(np.uint8).reshape(idx.numel(), augment.AUG_DTYPE.itemsize))
        aug_dev = raw.pin_memory().to(self.device, non_blocking=True)
        x = kernels.gather_augmented_batch(self.buf, off, sizes_dev, idx_dev, aug_dev, H, W, dtype, pad_value)
        return x, sizes


# ------------------------------------------------------------------------------------------------ the data set

class ResidentDataset:
    """One store (a unimodal model's inputs) or two (image and audio of the same pieces, sample n of both) and the targets: a host
    list of int64 token tensors, each with its <sos> and <eos>."""

    def __init__(self, images: Optional[ResidentStore] = None, audios: Optional[ResidentStore] = None, targets: Sequence[Tensor] = ()):
        self.stores = [s for s in (images, audios) if s is not None]
        if not self.stores:
            raise ValueError("ResidentDataset needs an image store, an audio store or both")
        self.targets = [torch.as_tensor(t, dtype=torch.int64).reshape(-1) for t in targets]
        if any(len(s) != len(self.targets) for s in self.stores):
            raise ValueError(f"stores of {[len(s) for s in self.stores]} samples for {len(self.targets)} targets")
        if any(t.numel() < 2 for t in self.targets):
            raise ValueError("a target holds at least <sos> and <eos>")
        for s in self.stores:
            s.freeze()

    @classmethod
    def from_raw_images(cls, raws: Sequence, img_height: Optional[int], targets: Sequence[Tensor], device=None) -> "ResidentDataset":
        """PIL images / uint8 arrays -> `image.preprocess_image` (gray, resize to img_height, / 255) -> a "u8" store."""
        from .image import preprocess_image
        store = ResidentStore("u8", device)
        for raw in raws:
            store.append(preprocess_image(raw, img_height, torch.float32, store.device))
        return cls(images=store, targets=targets)

    def __len__(self) -> int:
        return len(self.targets)

    def target_lens(self) -> List[int]:
        """Decoder positions per sample: len(y) - 1, the length of y_in and of y_out."""
        return [int(t.numel()) - 1 for t in self.targets]

    def batch(self, indices: Sequence[int], dtype: torch.dtype, records=None):
        """-> (x, sizes, y_in, y_out) for one store, (xi, sizes_i, xa, sizes_a, y_in, y_out) for two: the ragged batch forms of
        `Transformer.training_step` / `MultimodalTransformer.training_step`.  y_in = y[:-1], y_out = y[1:], padded with 0 to the
        batch's longest target, int64 on the host (`pad_batch_transcripts`, preprocessing.py:78-82).

        records: per STORE -- a sequence of len(stores) entries, each `augment.AUG_DTYPE` [B] or None (that store is gathered
        plainly); with one store the array itself will do.  The sizes returned for an augmented store are its records' extents."""
        indices = [int(i) for i in indices]
        if records is None:
            per_store = [None] * len(self.stores)
        elif isinstance(records, np.ndarray):
            per_store = [records]
        else:
            per_store = list(records)
        if len(per_store) != len(self.stores):
            raise ValueError(f"records for {len(per_store)} stores, the data set has {len(self.stores)}")
        out = []
        for s, r in zip(self.stores, per_store):
            out.extend(s.gather(indices, dtype) if r is None else s.gather(indices, dtype, records=r))
        ys = [self.targets[i] for i in indices]
        T = max(int(y.numel()) for y in ys) - 1
        y_in = torch.zeros((len(ys), T), dtype=torch.int64)
        y_out = torch.zeros((len(ys), T), dtype=torch.int64)
        for b, y in enumerate(ys):
            y_in[b, :y.numel() - 1], y_out[b, :y.numel() - 1] = y[:-1], y[1:]
        return tuple(out) + (y_in, y_out)

    def eval_batches(self, dtype: torch.dtype = torch.float32) -> Iterator[tuple]:
        """The items of `validation_step` / `evaluate`: (x [1, 1, h, w], y [1, L]) or (xi, xa, y), batch size 1, nothing padded."""
        for n, y in enumerate(self.targets):
            yield tuple(s.gather([n], dtype)[0] for s in self.stores) + (y.unsqueeze(0),)


# ------------------------------------------------------------------------------------------------ the bucketing plan (host only)

def _size_rows(sizes) -> List[List[int]]:
    rows = torch.as_tensor(sizes).reshape(-1, 2).tolist()
    return [[int(h), int(w)] for h, w in rows]


def plan_batches(sizes, batch_size: int, *, sizes2=None, target_lens: Optional[Sequence[int]] = None, max_padded_pixels: Optional[int] = None,
                 max_padded_tokens: Optional[int] = None, chunk_batches: int = 32, seed: int = 0, epoch: int = 0) -> List[List[int]]:
    """Batches of sample indices for one epoch, every sample exactly once.

    1. permute the N samples with torch.Generator().manual_seed(seed + epoch) (`ddp.shard_indices` seeds the same way);
    2. cut the permutation into chunks of chunk_batches * batch_size samples;
    3. sort each chunk, stably, by (width, height) of `sizes` (int [N, 2] = (h, w); for pairs the image table, `sizes2` the audio's);
    4. walk each chunk and close the batch when the next sample would make it break a limit: more than batch_size samples, more
       than max_padded_pixels pixels in the padded plane(s) (B * Hmax * Wmax; for pairs the two planes added), more than
       max_padded_tokens decoder positions (B * Tmax, `target_lens`).  A sample that breaks a limit on its own is a batch of one:
       nothing is ever dropped;
    5. shuffle the order of the batches with the same generator.

    chunk_batches = 1 without a budget: the batches are the consecutive slices of the permutation -- plain random batching.  Larger
    chunks trade randomness for less padding (DESIGN.md "Resident dataset and bucketed batches")."""
    if batch_size < 1 or chunk_batches < 1:
        raise ValueError("batch_size and chunk_batches must be at least 1")
    hw = _size_rows(sizes)
    N = len(hw)
    hw2 = _size_rows(sizes2) if sizes2 is not None else None
    if hw2 is not None and len(hw2) != N:
        raise ValueError(f"sizes2 has {len(hw2)} rows for {N} samples")
    if max_padded_tokens is not None and target_lens is None:
        raise ValueError("max_padded_tokens needs target_lens")
    tl = [int(t) for t in target_lens] if target_lens is not None else None
    if tl is not None and len(tl) != N:
        raise ValueError(f"target_lens has {len(tl)} entries for {N} samples")
    g = torch.Generator()
    g.manual_seed(seed + epoch)
    perm = torch.randperm(N, generator=g).tolist()
    chunk = chunk_batches * batch_size
    batches: List[List[int]] = []
    for c in range(0, N, chunk):
        cur: List[int] = []
        H = W = H2 = W2 = T = 0
        for n in sorted(perm[c:c + chunk], key=lambda n: (hw[n][1], hw[n][0])):
            nH, nW = max(H, hw[n][0]), max(W, hw[n][1])
            nH2, nW2 = (max(H2, hw2[n][0]), max(W2, hw2[n][1])) if hw2 is not None else (0, 0)
            nT = max(T, tl[n]) if tl is not None else 0
            B1 = len(cur) + 1
            full = (B1 > batch_size or (max_padded_pixels is not None and B1 * (nH * nW + nH2 * nW2) > max_padded_pixels)
                    or (max_padded_tokens is not None and B1 * nT > max_padded_tokens))
            if cur and full:
                batches.append(cur)
                cur = []
                nH, nW = hw[n]
                nH2, nW2 = hw2[n] if hw2 is not None else (0, 0)
                nT = tl[n] if tl is not None else 0
            cur.append(n)
            H, W, H2, W2, T = nH, nW, nH2, nW2, nT
        if cur:
            batches.append(cur)
    order = torch.randperm(len(batches), generator=g).tolist()
    return [batches[i] for i in order]


def shard_batches(plan: Sequence[List[int]], rank: int, world: int) -> List[List[int]]:
    """The batches of rank `rank`: the plan padded by wrap-around to a multiple of `world`, then r::world.  Every rank computes the
    same plan from the shared seed and gets the same number of steps, which `ddp.GradReducer` needs."""
    if not 0 <= rank < world:
        raise ValueError(f"rank {rank} of world {world}")
    if not plan:
        return []
    total = (len(plan) + world - 1) // world * world
    return [plan[i % len(plan)] for i in range(rank, total, world)]


def padded_ratio(plan: Sequence[Sequence[int]], sizes) -> float:
    """Real pixels / pixels of the padded planes (B * Hmax * Wmax per batch) over a plan."""
    hw = _size_rows(sizes)
    real = padded = 0
    for b in plan:
        real += sum(hw[n][0] * hw[n][1] for n in b)
        padded += len(b) * max(hw[n][0] for n in b) * max(hw[n][1] for n in b)
    return real / padded


# ------------------------------------------------------------------------------------------------ the loader

class ResidentLoader:
    """Training loader over a ResidentDataset: `plan_batches` per epoch (plan_kwargs: max_padded_pixels, max_padded_tokens,
    chunk_batches, seed; the size tables and target lengths come from the dataset), this rank's share by `shard_batches`, one
    `dataset.batch(indices, dtype)` per step -- no host pixel work between two steps.  `lightning_shim.Trainer.fit` calls
    `set_epoch(e)` and passes the device floats and the host integer tensors through as they are.

    augment / augment2 (`augment.ImageAugment`, `augment.SpecAugment` or anything with their `draw`): per-sample augmentation of the
    first / second store inside the gather, drawn afresh every epoch from plan_kwargs["seed"]; each batch carries its samples'
    records and its sizes are the augmented extents.  Both None: nothing new is launched, the loader is what it was.

    Data parallel: the batches of a plan differ in their number of tokens.  Each rank's loss is the mean over ITS batch's tokens
    and the gradient all-reduce averages the ranks' means, so a token of a short batch weighs more than one of a long batch in the
    same step (with equal-sized random batches the weights only differ by the targets' lengths).  Reweighting by token counts is
    not done."""

    def __init__(self, dataset: ResidentDataset, batch_size: int, dtype: torch.dtype, *, rank: Optional[int] = None, world: Optional[int] = None,
                 augment=None, augment2=None, **plan_kwargs):
        import torch.distributed as dist
        init = dist.is_available() and dist.is_initialized()
        self.dataset, self.batch_size, self.dtype = dataset, batch_size, dtype
        self.rank = rank if rank is not None else (dist.get_rank() if init else 0)
        self.world = world if world is not None else (dist.get_world_size() if init else 1)
        unknown = set(plan_kwargs) - {"max_padded_pixels", "max_padded_tokens", "chunk_batches", "seed"}
        if unknown:
            raise TypeError(f"unexpected plan arguments {sorted(unknown)}")
        if augment2 is not None and len(dataset.stores) < 2:
            raise ValueError("augment2 is for the second store; the data set has one")
        self.plan_kwargs = plan_kwargs
        self.augments = [augment, augment2][:len(dataset.stores)]           # the arguments (in here `augment` is not the module)
        self.epoch = 0
        self._cached = None
        self._records = None                # (epoch, [AUG_DTYPE [N] or None per store])

    def set_epoch(self, epoch: int) -> None:
        self.epoch = epoch

    def records(self) -> List[Optional[np.ndarray]]:
        """Per store: the records [N] of the current epoch (`augment.draw_all` with the plan's seed), None for a store without
        augmentation.  Record n depends on (seed, epoch, n, h_n, w_n) alone, so every rank holds the same table."""
        if self._records is None or self._records[0] != self.epoch:
            seed = self.plan_kwargs.get("seed", 0)
            self._records = (self.epoch, [None if a is None else augment.draw_all(a, seed, self.epoch, s.sizes)
                                          for a, s in zip(self.augments, self.dataset.stores)])
        return self._records[1]

    def plan(self) -> List[List[int]]:
        """This rank's batches of the current epoch.  With augmentation the plan is made on the AUGMENTED sizes of that epoch: the
        padded-pixel budget holds for the planes that are actually built."""
        if self._cached is None or self._cached[0] != self.epoch:
            stores = self.dataset.stores
            sizes = [s.sizes for s in stores]
            if any(a is not None for a in self.augments):
                sizes = [s if r is None else torch.from_numpy(augment.extents(r)) for s, r in zip(sizes, self.records())]
            full = plan_batches(sizes[0], self.batch_size, sizes2=sizes[1] if len(stores) > 1 else None,
                                target_lens=self.dataset.target_lens(), epoch=self.epoch, **self.plan_kwargs)
            self._cached = (self.epoch, shard_batches(full, self.rank, self.world))
        return self._cached[1]

    def __len__(self) -> int:
        return len(self.plan())

    def __iter__(self):
        if all(a is None for a in self.augments):
            for indices in self.plan():
                yield self.dataset.batch(indices, self.dtype)
            return
        plan, records = self.plan(), self.records()
        for indices in plan:
            yield self.dataset.batch(indices, self.dtype, records=[None if r is None else r[indices] for r in records])
