"""msw_inflate.hip on hand-built DEFLATE streams that no compressor emits.

tests/test_gpu_gz.py feeds the kernel zlib's own output; this file feeds it
the corpus of tests/deflate_writer.py (checked against zlib on the CPU by
tests/test_deflate_writer.py): match geometry at chosen positions of the
window, the ring and the flush, dynamic headers zlib never writes, block
framing, the member's end, the CRC kernel at every size, and one stream per
error status.  Valid members are inflated a family per call and compared byte
for byte with the token interpreter's output; every malformed member must
give zlib's diagnosis in the project's words and name its own index.
Run with -m gpu."""
import os

import pytest

import deflate_writer as dw
from mini_parallel_amd import MswError
from mini_parallel_amd.fastq import bgzf_inflate

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx1():
    """A context with 1 MiB inflate groups (MSW_GZ_GROUP_MB is read when the
    context is made): msw_bgzf_inflate allocates its group buffers per call,
    1 GiB of device and 1.1 GiB of pinned memory by default, and the error
    cases make one call each.  The larger families span several groups."""
    import torch  # noqa: F401  (as conftest's gpu_ctx: libmsw.so binds torch's HIP runtime)
    from mini_parallel_amd import Context
    old = os.environ.get("MSW_GZ_GROUP_MB")
    os.environ["MSW_GZ_GROUP_MB"] = "1"
    try:
        ctx = Context(0)
    finally:
        if old is None:
            del os.environ["MSW_GZ_GROUP_MB"]
        else:
            os.environ["MSW_GZ_GROUP_MB"] = old
    yield ctx
    ctx.close()


def first_wrong_member(cs, got):
    """Name the first member whose bytes differ (for the assertion message)."""
    p = 0
    for c in cs:
        if got[p:p + len(c.plain)] != c.plain:
            return c.name
        p += len(c.plain)
    return "length %d instead of %d" % (len(got), p)


@pytest.mark.parametrize("fam", list(dw.VALID_FAMILIES))
def test_valid_streams_byte_exact(ctx1, fam):
    """A: overlap sweep k lanes into a window (short matches emitted by the
    lanes, long ones through the walk and copy_near's reciprocal branch);
    W: a match alone in its window, so that lane j makes its byte j: every
    off = 0..63 of the window's off mod d multiply for d = 1..63, and d >= 64;
    B: ring and flush edges, first in a window, after two literals, in the
    serial walk and in the scalar step; C: far distances, matches reaching byte 0,
    a full 64 KiB member; D: random token streams in three encodings (fixed,
    15-bit random codes, mixed blocks); E: header forms; F: block framing;
    G: the member's end; H: output sizes 0..520 (the CRC kernel).  Which decode
    path takes the matches of A, W and B is asserted from a model of the token
    loop in tests/test_deflate_writer.py."""
    cs = dw.family(fam)
    blob, plain = dw.blob_of(cs)
    got = bgzf_inflate(ctx1, blob)
    assert got == plain, first_wrong_member(cs, got)


def test_valid_streams_in_one_default_group(gpu_ctx):
    """The small families again as one file through the session's context
    (the default group size: every member in one launch, a wave each)."""
    cs = [c for f in "AWEFGH" for c in dw.family(f)]
    blob, plain = dw.blob_of(cs)
    got = bgzf_inflate(gpu_ctx, blob)
    assert got == plain, first_wrong_member(cs, got)


@pytest.mark.parametrize("name", [c.name for c in dw.family("X")])
def test_malformed_member_is_diagnosed(ctx1, name):
    """One malformed member behind one to three valid ones: zlib's diagnosis in the
    project's words (deflate_writer.ZLIB_TO_TEXT), and the member's index."""
    c = {c.name: c for c in dw.family("X")}[name]
    blob, k = dw.error_blob(c)
    with pytest.raises(MswError) as e:
        bgzf_inflate(ctx1, blob)
    msg = str(e.value)
    if c.kind != "clen0":  # no deflate data at all: any error
        assert c.text and c.text in msg, msg
    assert "BGZF member %d " % k in msg, msg


@pytest.mark.parametrize("k", dw.H_BAD)
def test_crc_mismatch_names_its_member(ctx1, k):
    blob, idx = dw.h_bad_blob(k)
    with pytest.raises(MswError) as e:
        bgzf_inflate(ctx1, blob)
    assert "incorrect data check" in str(e.value) and "BGZF member %d " % idx in str(e.value), str(e.value)
