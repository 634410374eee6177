"""The shared weight image of the L0X training instance (reni_dev_train.inc: wimg_cell, wimg_tr_base; k_pack: PackDesc::swz), on the CPU.

One packed image per hidden layer serves the forward GEMM (ds_read_b128 of fragment (row block, k-step)) and the backward step's dX
GEMM (two ds_read_b64_tr_b16 per fragment (k block, row step) of W^T).  Two things are checked on a host-side model:

  * banks: 64 banks x 4 B, the lane groups of each instruction as the LDS serves them (ds_read_b128: four non-contiguous groups of
    16 lanes; ds_read_b64_tr_b16: the two 32-lane halves; the LDS-DMA lands lane-linear, 16 B per lane).  Every address of every
    lane of every fragment is enumerated and the extra cycles counted: zero for both kinds of read and for the landing pattern --
    and NOT zero for the transposing reads of the plain forward layout, which is why the image is swizzled;
  * values: the transposing reads applied to a packed, swizzled forward image give exactly the fragments of the packed backward
    image (8 x the forward image's transpose: Layout::consistent_bwd) divided by 8.

The functions below restate the device code's index arithmetic; the GPU test (test_gpu_shared_wimage.py) holds the kernel to it."""
import numpy as np
import pytest

H, NRB, NKS = 128, 4, 8
FRAG = 1024   # bytes per fragment: 64 cells of 16 B


def kfeat(ks, hi, e):  # reni_dev_common.inc, bf16: the k index of element e of lane half hi in k-step ks
    return 16 * ks + (e & 3) + 8 * (e >> 2) + 4 * hi


def wimg_cell(lane, ks, swz=True):  # 16-byte cell of lane's operand within fragment (., ks)
    return lane ^ ((((lane >> 5) << 2) | ((ks & 1) << 3)) if swz else 0)


def fwd_addr(rb, ks, lane, swz=True):  # byte address of the forward ds_read_b128 of lane
    return (rb * NKS + ks) * FRAG + wimg_cell(lane, ks, swz) * 16


def tr_addr(kb, s, q, lane, swz=True):
    """byte address lane hands to transposing read q (0, 1) of fragment (row block kb of W^T, k-step s): wimg_tr_base + immediates."""
    khi, g, u = lane >> 5, (lane >> 4) & 1, lane & 15
    h = u & 1
    x = (4 * h + 8 * g) if swz else 0
    base = g * 1024 + h * 512 + (((4 * khi + (u >> 2)) ^ x) << 4) + ((u >> 1) & 1) * 8
    if q:
        base ^= 128
    return base + kb * 2048 + (s >> 1) * 8192 + (s & 1) * 256


B128_GROUPS = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
B128_GROUPS += [[l + 32 for l in grp] for grp in B128_GROUPS]
HALVES = [list(range(32)), list(range(32, 64))]
DMA_GROUPS = [list(range(16 * k, 16 * k + 16)) for k in range(4)]


def extra_cycles(addrs, nbytes, groups):
    """LDS cycles beyond one per lane group: per group, a bank serves one distinct dword address per cycle (equal addresses broadcast)."""
    extra = 0
    for grp in groups:
        per_bank = {}
        for lane in grp:
            for d in range(nbytes // 4):
                a = addrs[lane] + 4 * d
                per_bank.setdefault((a // 4) % 64, set()).add(a)
        extra += max(len(v) for v in per_bank.values()) - 1
    return extra


def test_forward_reads_have_no_bank_conflict():
    for rb in range(NRB):
        for ks in range(NKS):
            addrs = [fwd_addr(rb, ks, lane) for lane in range(64)]
            assert sorted(addrs) == [(rb * NKS + ks) * FRAG + 16 * c for c in range(64)]   # a permutation of the fragment's cells
            assert extra_cycles(addrs, 16, B128_GROUPS) == 0


def test_transposing_reads_have_no_bank_conflict():
    for kb in range(NRB):
        for s in range(NKS):
            for q in range(2):
                addrs = [tr_addr(kb, s, q, lane) for lane in range(64)]
                assert all(a % 8 == 0 and 0 <= a < NRB * NKS * FRAG for a in addrs)
                assert extra_cycles(addrs, 8, HALVES) == 0


def test_plain_layout_would_conflict():
    # (what the swizzle is for: on the plain forward layout the two lane halves `hi` and the two k-steps of a 32-column group sit
    # 512 B and 1 KB apart -- the same banks -- and every transposing read is served in four cycles per half instead of one)
    addrs = [tr_addr(0, 0, 0, lane, swz=False) for lane in range(64)]
    assert extra_cycles(addrs, 8, HALVES) == 2 * 3


def test_dma_landing_pattern_has_no_bank_conflict():
    # the LDS-DMA writes the image as it lies in memory: instruction n lands lane l's 16 bytes at 1024 n + 16 l
    for n in range(NRB * NKS):
        assert extra_cycles([n * FRAG + 16 * lane for lane in range(64)], 16, DMA_GROUPS) == 0


def bf16_bits(x):  # float32 -> bf16 bit pattern, round to nearest even (what the device's conversion does for finite values)
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def bf16_val(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


def pack(W, scale, transposed, swz):
    """k_pack (pack_body) for one H x H matrix: the image as uint16 [fragment][cell][8]."""
    img = np.zeros((NRB * NKS, 64, 8), np.uint16)
    for rb in range(NRB):
        for ks in range(NKS):
            for lane in range(64):
                R, hi = 32 * rb + (lane & 31), lane >> 5
                v = [W[kfeat(ks, hi, e), R] if transposed else W[R, kfeat(ks, hi, e)] for e in range(8)]
                img[rb * NKS + ks, wimg_cell(lane, ks, swz)] = bf16_bits(np.float32(v) * np.float32(scale))
    return img


def tr_read(img_bytes, addrs):
    """ds_read_b64_tr_b16: per group of 16 lanes, lane 4 r + p supplies row r, columns 4 p .. 4 p + 3; lane i receives column i of the
    four rows, row r in its element r."""
    out = np.zeros((64, 4), np.uint16)
    for g0 in range(0, 64, 16):
        block = np.zeros((4, 16), np.uint16)
        for r in range(4):
            for p in range(4):
                a = addrs[g0 + 4 * r + p]
                block[r, 4 * p:4 * p + 4] = img_bytes[a // 2:a // 2 + 4]
        for i in range(16):
            out[g0 + i] = block[:, i]
    return out


@pytest.mark.parametrize("omega", [30.0, 1.0, 200.0])
def test_transposed_fragments_are_the_backward_image_over_8(omega):
    rng = np.random.default_rng(7)
    W = (rng.standard_normal((H, H)) * 0.1).astype(np.float32)
    W[0, 0], W[5, 77], W[127, 127] = 0.0, -3.0e-5, 2.5    # a zero, a small and a large weight
    scale = np.float32(omega) * np.float32(0.15915494309189535)
    fwd = pack(W, scale, transposed=False, swz=True)          # the shared image
    bwd = pack(W, scale * np.float32(8.0), transposed=True, swz=False)   # the W^T image of Layout::consistent_bwd
    flat = fwd.reshape(-1)
    for kb in range(NRB):
        for s in range(NKS):
            lo = tr_read(flat, [tr_addr(kb, s, 0, lane) for lane in range(64)])
            up = tr_read(flat, [tr_addr(kb, s, 1, lane) for lane in range(64)])
            got = bf16_val(np.concatenate([lo, up], axis=1))
            want = bf16_val(bwd[kb * NKS + s]) / np.float32(8.0)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (kb, s)
