"""Generates tests/golden/qmx_reference_codec.npz: what the REFERENCE QMX encoder (qmx_codec.hpp, compiled as-is into
oracle/_ref/libqmx_ref.so by oracle/Makefile) writes for
  - the 600 seeded blocks of tests/test_codecs_cpu.py::test_qmx_against_reference_codec (0..32 bits x four value shapes):
    values (600 x 128 u32), enc (their byte streams, concatenated), enc_off (601 offsets into enc);
  - the 128-value QMX rows of appendix_c.json: appendix_names, appendix_enc, appendix_off (the same layout).
Run where the reference is present (oracle/_ref built); the fixture travels, the reference does not."""
import json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import oracle as o

HERE = os.path.dirname(os.path.abspath(__file__))
o.build()
R = o.ref_qmx()
assert R is not None, "oracle/_ref/libqmx_ref.so missing (the reference is needed to generate this fixture)"


def ref_encode(v):
    buf = np.zeros(8192, dtype=np.uint8)
    ln = R.ref_qmx_encode(buf.ctypes.data, v.ctypes.data)
    out = np.zeros(640, dtype=np.uint32)
    R.ref_qmx_decode(out.ctypes.data, buf.ctypes.data, ln)
    assert np.array_equal(out[:128], v)
    return bytes(buf[:ln])


rng = np.random.default_rng(7)
values, enc = [], []
for it in range(600):
    mag = int(rng.integers(0, 33))
    kind = it % 4
    if kind == 0:
        v = rng.integers(0, 1 << mag, size=128, dtype=np.uint64)
    elif kind == 1:
        v = np.where(rng.random(128) < 0.9, rng.integers(0, 4, 128), rng.integers(0, 1 << mag, 128))
    elif kind == 2:
        v = np.repeat(rng.integers(0, 1 << mag, 32), 4) >> rng.integers(0, 8, 128)
    else:
        v = np.where(rng.random(128) < 0.7, 1, rng.integers(0, 1 << (mag // 2), 128))
    v = np.ascontiguousarray(v, dtype=np.uint32)
    values.append(v)
    enc.append(ref_encode(v))
names, app = [], []
for case in json.load(open(os.path.join(HERE, "appendix_c.json")))["blocks"]:
    if case["codec"] == "block_qmx" and len(case["values"]) == 128:
        names.append(case["name"])
        app.append(ref_encode(np.ascontiguousarray(case["values"], dtype=np.uint32)))
off = lambda bs: np.cumsum([0] + [len(b) for b in bs]).astype(np.uint32)
path = os.path.join(HERE, "qmx_reference_codec.npz")
np.savez_compressed(path, values=np.stack(values), enc=np.frombuffer(b"".join(enc), dtype=np.uint8), enc_off=off(enc),
                    appendix_names=np.array(names), appendix_enc=np.frombuffer(b"".join(app), dtype=np.uint8), appendix_off=off(app))
print(path, len(values), len(names), os.path.getsize(path))
