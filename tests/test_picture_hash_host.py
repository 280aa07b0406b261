"""CPU: the host models of the decoded-picture-hash SEI's CRC and checksum (H.265 Annex D) that the GPU tests compare against, and the
stream writer's oh_stream_add_hash read back through annexb.picture_hash (and, where oracle/_ref is built, by the reference decoder)."""
import binascii

import numpy as np
import pytest

import picture_hash as PH
import refdec
import streamgen


def test_crc_transcription_is_crc16_aug_ccitt():
    rng = np.random.default_rng(5)
    planes = [rng.integers(0, 256, (11, 37), dtype=np.uint8), rng.integers(0, 1 << 10, (9, 23), dtype=np.uint16),
              rng.integers(0, 1 << 12, (4, 300), dtype=np.uint16), np.zeros((2, 3), np.uint8)]
    for pl in planes:
        data = PH.packed(pl)
        assert PH.crc_annex_d(data) == binascii.crc_hqx(data, 0x1D0F) == PH.crc(pl)
    assert PH.packed(np.array([[0x0102]], np.uint16)) == b"\x02\x01"                 # low byte first
    assert PH.crc_annex_d(b"123456789") == 0xE5CC and binascii.crc_hqx(b"123456789", 0x1D0F) == 0xE5CC
    assert PH.crc_annex_d(b"") == 0x1D0F


@pytest.mark.parametrize("h,w,bd", [(5, 300, 8), (4, 520, 10), (3, 17, 12), (270, 3, 9), (8, 8, 8)])
def test_checksum_loop_equals_vectorised(h, w, bd):
    rng = np.random.default_rng(h * 1000 + w + bd)
    pl = rng.integers(0, 1 << bd, (h, w), dtype=np.uint8 if bd == 8 else np.uint16)
    assert PH.checksum_loop(pl, bd) == PH.checksum(pl, bd)


def test_checksum_wraps_mod_2_32():
    """a 7680x4320 12-bit plane of 4095s sums to more than 2^32: the model keeps the low 32 bits (HM's & 0xffffffff), as an
    accumulation that wraps as it goes does"""
    pl = np.full((4320, 7680), 4095, np.uint16)
    x = np.arange(7680, dtype=np.int64)[None, :]
    y = np.arange(4320, dtype=np.int64)[:, None]
    mask = (x & 0xFF) ^ (y & 0xFF) ^ (x >> 8) ^ (y >> 8)
    terms = np.concatenate([(0xFF ^ mask).ravel(), (0x0F ^ mask).ravel()])
    exact = int(terms.sum())
    assert exact > 1 << 32
    assert PH.checksum(pl, 12) == exact % (1 << 32) == int(terms.astype(np.uint32).sum(dtype=np.uint32))


VALUES = {
    1: [[0x0000, 0x0003, 0x0000], [0xFFFF, 0x0000, 0x0001], [0x1234, 0x0003, 0x0300]],
    2: [[0x00000000, 0x00000003, 0x00000001], [0xFFFFFFFF, 0x00000300, 0x00030000], [0x12345678, 0x00000000, 0x9ABCDEF0]],
}


@pytest.mark.parametrize("hash_type", [1, 2], ids=["crc", "checksum"])
def test_add_hash_sei_reads_back(hash_type):
    """the SEIs that oh_stream_add_hash writes come back exactly through oh_sei_picture_hash — values with zero runs need emulation
    prevention — and stay in their picture's access unit"""
    data, aus = streamgen.write_stream(64, 64, 3, n_pictures=3, gop=2)
    vals = VALUES[hash_type]
    out, aus2 = PH.add_hash(data, aus, hash_type, vals)
    assert b"\x00\x00\x03" in out[aus2[0][0]:aus2[0][1]]
    assert [tuple(a) for a in refdec.split_access_units(out)] == [tuple(a) for a in aus2]
    assert PH.sei_hashes(out, aus2) == [(hash_type, v) for v in vals]
    for k in range(3):                                        # the picture's own bytes are untouched, the SEI follows them
        assert out[aus2[k][0]:aus2[k][0] + aus[k][1] - aus[k][0]] == data[aus[k][0]:aus[k][1]]


def test_add_hash_sizes_and_bad_type():
    data, aus = streamgen.write_stream(64, 64, 4, n_pictures=2, gop=1)
    for t, per in ((1, 2), (2, 4)):
        vals = [[0x1111 * (c + 1) for c in range(3)] for _ in aus]          # no zero bytes: no emulation prevention
        out, _ = PH.add_hash(data, aus, t, vals)
        assert len(out) == len(data) + len(aus) * (4 + 2 + 3 + 3 * per + 1)    # start code, NAL header, type/size/hash_type, values, trailing
    with pytest.raises(ValueError):
        PH.add_hash(data, aus, 3, [[0, 0, 0]] * len(aus))


def test_type0_is_add_md5():
    import hashlib
    data, aus = streamgen.write_stream(264, 200, 21, n_pictures=3, gop=2, bit_depth=10)
    digests = [[hashlib.md5(bytes([k, c])).digest() for c in range(3)] for k in range(3)]
    digests[1][0] = b"\x00\x00\x00\x01" + digests[1][0][4:]
    assert PH.add_hash(data, aus, 0, digests) == streamgen.add_md5(data, aus, digests)


need_ref = pytest.mark.skipif(not refdec.have_refdec(), reason="reference tree / oracle/_ref not present")


@need_ref
@pytest.mark.parametrize("hash_type", [1, 2], ids=["crc", "checksum"])
def test_reference_decodes_crc_and_checksum_streams_unchanged(hash_type):
    """the reference reads CRC and checksum SEIs and drops them (hevc_sei.c:42-47): the pictures are those of the stream without
    them, and it reports no MD5 verdict and no error"""
    data, aus = streamgen.write_stream(264, 200, 22, n_pictures=3, gop=2, bit_depth=10)
    pics = refdec.decode(data)
    rank = streamgen.output_rank(3, 2)
    vals = [PH.picture_hash(pics[rank[k]], 10, hash_type)[1] for k in range(3)]
    with_sei, _ = PH.add_hash(data, aus, hash_type, vals)
    with refdec.captured_stderr() as log:
        again = refdec.decode(with_sei, check_md5=True)
    assert len(again) == len(pics)
    assert all(np.array_equal(a[c], b[c]) for a, b in zip(pics, again) for c in range(3))
    assert "MD5" not in log.text and "rror" not in log.text, log.text[-2000:]
