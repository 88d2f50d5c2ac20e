"""What the convolution kernels share (csrc/conv_tile.h: tile order, LDS row contract, pixel decomposition, fp16 clamp and hi / lo
rounding) compiled for the host and checked without a GPU: the functions the eight convolution units call."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HOST_DRIVER = r"""
#include "conv_tile.h"
#include <string.h>
extern "C" {
void ct_xcd_order(int n, int* out) { for (int q = 0; q < n; ++q) out[q] = xcd_tile(q, n); }
int ct_act_key(int row) { return act_key(row); }
int ct_w_key(int row, int blk) { return w_key(row, blk); }
int ct_src_chunk(int lchk, int key) { return src_chunk(lchk, key); }
int ct_chunk_f16(int d) { return chunk_f16(d); }
long long ct_chunk_split(int d, long long lo) { return chunk_split(d, lo); }
int ct_frag_row(int fi, int i, int blk) { return frag_row(fi, i, blk); }
int ct_frag_off(int fq, int fkey, int kk) { return frag_off(fq, fkey, kk); }
// every pixel m < M as (x, y, n), and every sum m0 + r (m0, r < M) through the carry form from the decompositions of m0 and r
void ct_pix_all(int Wo, int Ho, int M, int* of, int* add) {
  for (int m = 0; m < M; ++m) { const Pix p = pix_of(m, Wo, Ho); of[3 * m] = p.x; of[3 * m + 1] = p.y; of[3 * m + 2] = p.n; }
  for (int m0 = 0; m0 < M; ++m0)
    for (int r = 0; r < M; ++r) {
      const Pix a = pix_of(m0, Wo, Ho), b = pix_of(r, Wo, Ho);
      const Pix s = pix_add(a.x, a.y, a.n, b.x, b.y, b.n, Wo, Ho);
      int* o = add + 3 * (m0 * M + r);
      o[0] = s.x; o[1] = s.y; o[2] = s.n;
    }
}
#if !defined(CT_NO_F16)
void ct_round(const float* f, int n, float* clamp, float* clamp_pos, unsigned short* h, unsigned short* l) {
  for (int i = 0; i < n; ++i) {
    clamp[i] = clamp_h16(f[i]);
    clamp_pos[i] = clamp_h16_pos(f[i]);
    const HiLo s = split_round(f[i]);
    memcpy(h + i, &s.h, 2);
    memcpy(l + i, &s.l, 2);
  }
}
#endif
}
"""


def _compilers():
    rocm_clang = "/opt/rocm/lib/llvm/bin/clang++"
    found = [shutil.which(c) for c in ("g++", "c++", "clang++")] + [rocm_clang if os.path.exists(rocm_clang) else None]
    return [c for c in found if c]


@pytest.fixture(scope="module")
def tile(tmp_path_factory):
    """csrc/conv_tile.h behind the driver above, compiled for the host by the first compiler that knows _Float16; by any compiler without
    the rounding part (lib.has_f16 False) when none does."""
    cxxs = _compilers()
    if not cxxs:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("conv_tile_host")
    (d / "driver.cpp").write_text(HOST_DRIVER)
    so = str(d / "libconv_tile_host.so")
    base = ["-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", os.path.join(ROOT, "proj_roadsurf_amd", "csrc"), str(d / "driver.cpp"), "-o", so]
    has_f16 = False
    for cxx in cxxs:
        if subprocess.run([cxx] + base, capture_output=True).returncode == 0:
            has_f16 = True
            break
    if not has_f16:
        subprocess.run([cxxs[0], "-DCT_NO_F16"] + base, check=True)
    lib = C.CDLL(so)
    lib.ct_chunk_split.argtypes, lib.ct_chunk_split.restype = [C.c_int, C.c_longlong], C.c_longlong
    lib.has_f16 = has_f16
    return lib


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def test_xcd_tile_is_a_permutation_in_eight_contiguous_runs(tile):
    """For every n from 1 to 4096: xcd_tile(., n) is a permutation of 0 .. n-1; positions q and q + 8 (the same XCD) get consecutive
    logical tiles; the eight residue classes are eight contiguous runs, in class order, whose lengths differ by at most one."""
    for n in range(1, 4097):
        order = np.zeros(n, np.int32)
        tile.ct_xcd_order(n, _ptr(order))
        assert np.array_equal(np.sort(order), np.arange(n)), n
        assert np.array_equal(order[8:], order[:-8] + 1), n
        runs = [order[x::8] for x in range(8)]
        lens = [len(r) for r in runs]
        assert max(lens) - min(lens) <= 1, (n, lens)
        start = 0
        for r in runs:      # class x starts where class x - 1 ended
            assert len(r) == 0 or r[0] == start, (n, start)
            start += len(r)
        assert start == n


# (block height = rows one value of fi >> 2 reads, who uses it)
BLOCKS = [(4, "MI = 1: conv_igemm's 16-row head tile"), (16, "MI = 4: the 64-row wave tiles; MIB = 4: the 64-wide bottleneck; bneck_*'s `row >> 4`"),
          (32, "MIB = 8: the 128-wide bottleneck"), (8, "conv_wide1x1_split's 32-row pass slices")]
LO = 1 << 20      # lo-plane offset of the split form (elements)


def _stage(tile, rows, key_of, split):
    """The staging write: waves of 64 lanes write 8-row pieces lane-linearly (lane l: 16 bytes at piece base + 16 l); what lands in slot s of
    row r is the source element offset of the lane's chunk."""
    lds = np.full((rows, 8), -1, np.int64)
    for r0 in range(0, rows, 8):
        for lane in range(64):
            lrow, lchk = lane >> 3, lane & 7
            d = tile.ct_src_chunk(lchk, key_of(r0 + lrow))
            byte = r0 * 128 + lane * 16
            lds[byte // 128, (byte % 128) // 16] = tile.ct_chunk_split(d, LO) if split else tile.ct_chunk_f16(d)
    assert (lds >= 0).all()
    return lds


def _want(fq, kk, split):
    """first K element (offset in the source row) of the fragment of lane k-slice fq in half-step kk"""
    return (kk * LO + fq * 8) if split else (kk * 32 + fq * 8)


@pytest.mark.parametrize("split", [False, True], ids=["fp16", "split"])
def test_fragment_reads_get_the_k_elements_the_staging_wrote(tile, split):
    """The row contract, exhaustively: all 64 lanes, the block heights the kernels use, tiles of 16 to 256 rows.  Weights: the lane reading
    block i of wave tile w gets, at frag_off(fq, fkey, kk) of row frag_row(fi, i, blk), K elements kk * 32 + fq * 8 .. + 7 of that row (fp16
    form) or its hi (kk = 0) / lo (kk = 1) halfs fq * 8 .. + 7 (split form); the rows a wave tile's lanes read are a permutation of its rows,
    and the MFMA leaves lane k-slice fq with the 4 MI consecutive channels fq * blk .. + blk - 1.  Pixels: the same for row 16 j + fi."""
    checked = 0
    for blk, _who in BLOCKS:
        mi = blk // 4
        for rows in range(16, 257, 16):
            if rows % (4 * blk):
                continue
            lds = _stage(tile, rows, lambda r: tile.ct_w_key(r, blk), split)
            for w in range(rows // (4 * blk)):
                seen = []
                for lane in range(64):
                    fi, fq, fkey = lane & 15, lane >> 4, lane & 7
                    for i in range(mi):
                        row = w * 4 * blk + tile.ct_frag_row(fi, i, blk)
                        assert tile.ct_w_key(row, blk) == fkey, (blk, rows, lane, i)
                        for kk in range(2):
                            off = tile.ct_frag_off(fq, fkey, kk)
                            assert off % 16 == 0 and 0 <= off < 128
                            assert lds[row, off // 16] == _want(fq, kk, split), (blk, rows, lane, i, kk)
                            checked += 1
                        if fq == 0:
                            seen.append(row - w * 4 * blk)
                assert sorted(seen) == list(range(4 * blk)), (blk, rows, w)
            # D row a of block i (held by lane k-slice a >> 2 as element a & 3) is weight row frag_row(a, i, blk)
            for g in range(4):
                assert [tile.ct_frag_row(4 * g + r, i, blk) for i in range(mi) for r in range(4)] == list(range(g * blk, (g + 1) * blk))
    for rows in range(16, 257, 16):
        lds = _stage(tile, rows, tile.ct_act_key, split)
        for j in range(rows // 16):
            for lane in range(64):
                fi, fq, fkey = lane & 15, lane >> 4, lane & 7
                row = 16 * j + fi
                assert tile.ct_act_key(row) == fkey
                for kk in range(2):
                    assert lds[row, tile.ct_frag_off(fq, fkey, kk) // 16] == _want(fq, kk, split), (rows, lane, j, kk)
                    checked += 1
    assert checked > 50000


def test_pix_of_and_pix_add_agree_with_divmod(tile):
    """Maps from 1 x 1 to 7 x 5 with 1 to 3 images: pix_of(m) for every m, and pix_add for every pair (m0, r) of pixels of the map -- every
    offset it admits has rx < Wo and ry < Ho, which the decomposition of any r gives -- against Python's divmod."""
    for Wo in range(1, 8):
        for Ho in range(1, 6):
            for N in range(1, 4):
                M = N * Ho * Wo
                of, add = np.zeros((M, 3), np.int32), np.zeros((M, M, 3), np.int32)
                tile.ct_pix_all(Wo, Ho, M, _ptr(of), _ptr(add))
                for m in range(M):
                    t, x = divmod(m, Wo)
                    n, y = divmod(t, Ho)
                    assert of[m].tolist() == [x, y, n], (Wo, Ho, m)
                s = np.arange(M)[:, None] + np.arange(M)[None, :]
                want = np.stack([s % Wo, (s // Wo) % Ho, s // (Wo * Ho)], -1)
                assert np.array_equal(add, want), (Wo, Ho, N)


def test_clamps_and_split_round_equal_numpy_bit_for_bit(tile):
    """clamp_h16 / clamp_h16_pos / split_round on 100 000 random fp32 values over 1e-8 .. 1e6 in both signs plus the edges, against numpy
    (np.float16(f), np.float16(f - np.float32(h))).  A NaN passes through both clamps (the kernels' ternaries compare false) and splits
    into (NaN, NaN)."""
    if not tile.has_f16:
        pytest.skip("no host compiler with _Float16")
    rng = np.random.default_rng(7)
    mag = np.exp(rng.uniform(np.log(1e-8), np.log(1e6), 100000)).astype(np.float32)
    rnd = mag * rng.choice(np.array([-1.0, 1.0], np.float32), mag.shape)
    above = np.nextafter(np.float32(65504), np.float32(np.inf))
    sub = np.array([2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -24, 2.0 ** -14 - 2.0 ** -24, 2.0 ** -15, 6.1e-5], np.float32)
    edges = np.array([65504, -65504, 65520, -65520, above, -above, np.inf, -np.inf, np.nan, 0.0, -0.0], np.float32)
    f = np.concatenate([rnd, edges, sub, -sub]).astype(np.float32)
    n = len(f)
    cl, cp = np.zeros(n, np.float32), np.zeros(n, np.float32)
    h, l = np.zeros(n, np.uint16), np.zeros(n, np.uint16)
    tile.ct_round(_ptr(f), n, _ptr(cl), _ptr(cp), _ptr(h), _ptr(l))
    nan = np.isnan(f)
    assert nan.sum() == 1
    with np.errstate(invalid="ignore", over="ignore"):
        want_cl = np.where(f > 65504, np.float32(65504), np.where(f < -65504, np.float32(-65504), f)).astype(np.float32)
        want_cp = np.where(f > 65504, np.float32(65504), f).astype(np.float32)
        want_h = f.astype(np.float16)
        want_l = (f - want_h.astype(np.float32)).astype(np.float16)
    assert np.isnan(cl[nan]).all() and np.isnan(cp[nan]).all()
    assert np.array_equal(cl[~nan].view(np.uint32), want_cl[~nan].view(np.uint32))
    assert np.array_equal(cp[~nan].view(np.uint32), want_cp[~nan].view(np.uint32))
    assert cl[n - len(sub) * 2 - len(edges):][:8].tolist() == [65504, -65504, 65504, -65504, 65504, -65504, 65504, -65504]
    assert cp[n - len(sub) * 2 - len(edges):][:8].tolist() == [65504, -65504, 65504, -65520, 65504, float(-above), 65504, -np.inf]
    hn, ln = np.isnan(want_h), np.isnan(want_l)      # NaN in: (NaN, NaN); +-inf in: (+-inf, NaN)
    assert np.array_equal(np.isnan(h.view(np.float16)), hn) and np.array_equal(np.isnan(l.view(np.float16)), ln)
    assert hn.sum() == 1 and ln.sum() == 3
    assert np.array_equal(h[~hn], want_h.view(np.uint16)[~hn])
    assert np.array_equal(l[~ln], want_l.view(np.uint16)[~ln])
