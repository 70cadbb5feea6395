#!/usr/bin/env python3
"""Generate tests/golden/reference_pooling_outputs.npz: outputs of the COMPILED REFERENCE
(oracle/_ref/libqnnpack_ref.so) for a spread of the max / average pooling cases of tests/_pooling.py (every 61st case of
each restated reference test, the extra cases without device-only fields, the bench rows at batch 1).
Inputs are not stored: they are regenerated from the case name's seed, and their CRC-32 pins that. Every output is
pinned by its CRC-32; outputs of up to 1 KiB are also stored whole (concatenated, with offsets per case), so that a
mismatch there can be shown byte by byte. Kept small: the file lives in the repository.
Run in the build container:  python tests/golden/generate_golden_pooling.py"""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _pooling as pl  # noqa: E402
from oracle import ref  # noqa: E402


FULL_BYTES = 1024     # outputs up to this size are stored whole; every output is pinned by its CRC-32


def golden_cases():
    cases = pl.thin(pl.reference_max_cases(), 61) + pl.thin(pl.reference_avg_cases(), 61)
    cases += [c for c in pl.extra_cases() if not (c.misalign_in or c.misalign_out or c.host)]
    cases += pl.bench_cases(1)
    return cases


def main():
    lib = ref.lib()
    cases = golden_cases()
    names, input_crc, output_crc, offsets, chunks = [], [], [], [0], []
    for case in cases:
        x = pl.input_tensor(case)
        outs, _ = pl.run(lib, case, x)
        names.append(case.name)
        input_crc.append(zlib.crc32(x.tobytes()))
        output_crc.append([zlib.crc32(o.tobytes()) for o in outs] + [0] * (2 - len(outs)))
        full = [o for o in outs if o.size <= FULL_BYTES] if all(o.size <= FULL_BYTES for o in outs) else []
        chunks += full
        offsets.append(offsets[-1] + sum(o.size for o in full))
    path = os.path.join(HERE, "reference_pooling_outputs.npz")
    np.savez_compressed(path, names=np.array(names), input_crc32=np.array(input_crc, dtype=np.uint32),
                        output_crc32=np.array(output_crc, dtype=np.uint32),
                        output_count=np.array([len(c.geometries()) for c in cases], dtype=np.uint8),
                        output_offsets=np.array(offsets, dtype=np.int64),
                        output_bytes=np.concatenate(chunks) if chunks else np.zeros(0, np.uint8))
    print(f"{len(cases)} pooling cases ->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
