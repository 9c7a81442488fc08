"""What the device codecs (flac_gpu, vorbis_gpu, mp3_gpu) share.

Each of those modules gives the batched corpus path (aa_amd.batch) the same
functions: ``sniff(buf, size)``, ``index_slot(buf, size) -> Slotted | None``,
``decode_batch(scratch, items, byte_bases, out_bases, comp, s16, device,
stream) -> positions of the files the device does not vouch for`` and
``host_samples(decoded) -> mono float32``.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

# A file the batch path decodes on the device, as it lies in its pinned slot:
# the codec's ``index``, the slot's first ``payload_bytes`` bytes (what crosses
# PCIe), and the ``n_in`` frames of ``channels`` samples at ``sr_in`` it decodes to.
Slotted = namedtuple("Slotted", "index payload_bytes n_in channels sr_in")


def u8(data) -> np.ndarray:
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data, dtype=np.uint8)
    return np.frombuffer(data, np.uint8)


def read_bytes(data_or_path):
    """The bytes themselves, or those of the file at a path."""
    if isinstance(data_or_path, (bytes, bytearray, memoryview, np.ndarray)):
        return data_or_path
    with open(data_or_path, "rb") as f:
        return f.read()


def to_device(table, device):
    """A host table (records of a structured dtype, or bytes) as device bytes."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(table).view(np.uint8).reshape(-1).copy())
    return t.to(device)


def slot_stream(ix, fits_batch):
    """Slotted of an index with one ``stream`` record and a ``payload`` (Vorbis,
    MP3), or None: no index, no frames, or a file ``fits_batch`` keeps on the host."""
    if ix is None or int(ix.stream["frames"][0]) <= 0 or not fits_batch(ix):
        return None
    st = ix.stream[0]
    return Slotted(ix, int(ix.payload.size), int(st["frames"]), int(st["channels"]), int(st["sample_rate"]))


def reread_samples(decoded):
    """host_samples of a codec whose index writes its payload over the file in
    the slot (Vorbis, MP3): the file again, through audio.decode."""
    from .audio import decode
    return decode(decoded.path)[0]


def groups_under(needs, cap):
    """Consecutive groups of range(len(needs)), each summing to at most ``cap``
    (a single item above the cap goes alone); no group is empty."""
    groups, size = [], 0
    for k, need in enumerate(needs):
        if not groups or size + need > cap:
            groups.append([])
            size = 0
        groups[-1].append(k)
        size += need
    return groups
