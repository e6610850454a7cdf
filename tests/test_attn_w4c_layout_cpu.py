"""CPU: the register / LDS layout of flash_attn_fwd_w4c_nm_kernel (gen3c_amd/csrc/attention_w4c.hpp), modelled lane by lane.

The kernel computes S^T = K Q^T and O^T = V^T P^T with v_mfma_f32_16x16x32_bf16, whose operand layout is (cdna_hip_programming.md, section 3):
  A: lane l holds A[row l & 15][k = 8 (l >> 4) + j], j < 8;   B: lane l holds B[k = 8 (l >> 4) + j][col l & 15];   D: register r of lane l is D[4 (l >> 4) + r][l & 15].
The kernel's claim: if row 4 g + r of key block b of 32-key group G of the K fragment loads physical key 32 G + 8 g + 4 b + r, then packing the D registers of
blocks b = 0, 1 of a lane in order gives exactly the P.V B operand (keys 32 G + 8 g .. + 7 of query l & 15), with V^T read in natural key order and no
cross-lane move. This file follows lane / register -> (key, query, dim) through the LDS-DMA image, the fragment reads, QK^T, the pack, P.V and the
epilogue's store index, with the addressing formulas copied from the kernel, and shows that the composition is the identity: the modelled kernel
returns K Q^T and V^T P^T of the plain matrices, exactly (integer data). It also checks what the kernel's own K swizzle is for: every ds_read_b128 of a
K or V^T fragment is free of LDS bank conflicts."""
import numpy as np

HD, KVB, LANES = 128, 64, 64
# lane groups of one ds_read_b128 (MI355X_MICROARCH.md, LDS): only lanes of one group conflict, on the 16-byte slot (address / 16) mod 16
B128_GROUPS = [[*range(0, 4), *range(12, 16), *range(20, 28)], [*range(4, 12), *range(16, 20), *range(28, 32)],
               [*range(32, 36), *range(44, 48), *range(52, 60)], [*range(36, 44), *range(48, 52), *range(60, 64)]]


def kswz(row):  # w4c_kswz
    return (row & 3) | (((row >> 3) & 3) << 2)


def k_off(row, chunk):  # w4c_k_off: element offset inside a [64][128] K stage
    return row * HD + ((chunk ^ kswz(row)) << 3)


def v_off(row, chunk):  # v_off of attention.hip: element offset inside a [128][64] V^T stage
    return row * KVB + ((chunk ^ ((row >> 1) & 7)) << 3)


def lds_dma_images(K, Vt):
    """The stage images the kernel's LDS-DMA writes: destination linear in (piece, thread), source chunk permuted (dma_off of the kernel)."""
    sK, sV = np.zeros(KVB * HD, K.dtype), np.zeros(HD * KVB, Vt.dtype)
    for j in range(4):
        for tid in range(256):
            row, src_chunk = (tid >> 4) + 16 * j, (tid & 15) ^ kswz((tid >> 4) + 16 * j)
            dst = 256 * 8 * j + tid * 8  # elements: piece j, then 16 bytes per thread
            sK[dst:dst + 8] = K[row, 8 * src_chunk:8 * src_chunk + 8]
            row, src_chunk = (tid >> 3) + 32 * j, (tid & 7) ^ (((tid >> 3) >> 1) & 7)
            sV[dst:dst + 8] = Vt[row, 8 * src_chunk:8 * src_chunk + 8]
    return sK, sV


def k_frag_addr(lane, ks, kb):  # kaddr[ks][kb & 1] + 8192 (kb >> 1) of the kernel, in elements
    l15, g = lane & 15, lane >> 4
    return k_off(32 * (kb >> 1) + 8 * (l15 >> 2) + (l15 & 3) + 4 * (kb & 1), 4 * ks + g)


def v_frag_addr(lane, G, d8):  # vaddr[G] + 2048 d8 of the kernel, in elements
    return v_off(16 * d8 + (lane & 15), 4 * G + (lane >> 4))


def mfma_16x16x32(a_frag, b_frag, acc):
    """a_frag, b_frag: [64 lanes][8]; acc: [64 lanes][4]. The instruction's own lane mapping."""
    A, Bm = np.zeros((16, 32), a_frag.dtype), np.zeros((32, 16), a_frag.dtype)
    for l in range(LANES):
        A[l & 15, 8 * (l >> 4):8 * (l >> 4) + 8] = a_frag[l]
        Bm[8 * (l >> 4):8 * (l >> 4) + 8, l & 15] = b_frag[l]
    D = A @ Bm
    out = acc.copy()
    for l in range(LANES):
        for r in range(4):
            out[l, r] += D[4 * (l >> 4) + r, l & 15]
    return out


def test_k_fragment_rows_give_each_lane_its_eight_keys():
    for G in range(2):
        for g in range(4):
            keys = []
            for b in range(2):  # D register r of lane group g in block b = A row 4 g + r = the key the lanes with l15 = 4 g + r loaded
                for r in range(4):
                    l15 = 4 * g + r
                    keys.append(32 * G + 8 * (l15 >> 2) + (l15 & 3) + 4 * b)
            assert keys == list(range(32 * G + 8 * g, 32 * G + 8 * g + 8))  # = the P.V B operand's keys 8 g + j of the group, in order


def test_one_tile_through_the_modelled_kernel_is_the_plain_product():
    rng = np.random.default_rng(5)
    K = rng.integers(-3, 4, (KVB, HD)).astype(np.int64)
    Vt = rng.integers(-3, 4, (HD, KVB)).astype(np.int64)
    Q = rng.integers(-3, 4, (64, HD)).astype(np.int64)  # one wave's 64 queries
    sK, sV = lds_dma_images(K, Vt)
    lanes = np.arange(LANES)
    # Q fragment (qb, ks): lane = query 16 qb + l15, dims 32 ks + 8 g .. + 7
    qfrag = {(qb, ks): np.stack([Q[16 * qb + (l & 15), 32 * ks + 8 * (l >> 4):32 * ks + 8 * (l >> 4) + 8] for l in lanes]) for qb in range(4) for ks in range(4)}
    # region A: group I = (kb = I & 3, ks = I >> 2), four MFMAs per K fragment
    S = {(kb, qb): np.zeros((LANES, 4), np.int64) for kb in range(4) for qb in range(4)}
    for I in range(16):
        kb, ks = I & 3, I >> 2
        kfrag = np.stack([sK[k_frag_addr(l, ks, kb):k_frag_addr(l, ks, kb) + 8] for l in lanes])
        for qb in range(4):
            S[kb, qb] = mfma_16x16x32(kfrag, qfrag[qb, ks], S[kb, qb])
    # every score sits where the kernel's epilogue / pack assume: lane l, block (kb, qb), register r = key 32 G + 8 g + 4 b + r, query 16 qb + l15
    ST = K @ Q.T
    for (kb, qb), blk in S.items():
        for l in lanes:
            for r in range(4):
                assert blk[l, r] == ST[32 * (kb >> 1) + 8 * (l >> 4) + 4 * (kb & 1) + r, 16 * qb + (l & 15)]
    # pair units: u -> (G, qb, b, pr), P dword 2 b + pr of pb[G][qb] = registers 2 pr, 2 pr + 1 of S[2 G + b][qb] (here P = S: any elementwise function commutes)
    P = {(G, qb): np.zeros((LANES, 8), np.int64) for G in range(2) for qb in range(4)}
    for u in range(32):
        G, qb, b, pr = u >> 4, (u >> 2) & 3, (u >> 1) & 1, u & 1
        P[G, qb][:, 2 * (2 * b + pr)] = S[2 * G + b, qb][:, 2 * pr]
        P[G, qb][:, 2 * (2 * b + pr) + 1] = S[2 * G + b, qb][:, 2 * pr + 1]
    # region B: group I = (G = I >> 3, d8 = I & 7), four MFMAs per V^T fragment into O^T block (d8, qb)
    O = {(d8, qb): np.zeros((LANES, 4), np.int64) for d8 in range(8) for qb in range(4)}
    for I in range(16):
        G, d8 = I >> 3, I & 7
        vfrag = np.stack([sV[v_frag_addr(l, G, d8):v_frag_addr(l, G, d8) + 8] for l in lanes])
        for qb in range(4):
            O[d8, qb] = mfma_16x16x32(vfrag, P[G, qb], O[d8, qb])
    # epilogue: register r of block (d8, qb) in lane l is stored to output dim 16 d8 + 4 g + r of query 16 qb + l15
    out = np.zeros((64, HD), np.int64)
    for (d8, qb), blk in O.items():
        for l in lanes:
            out[16 * qb + (l & 15), 16 * d8 + 4 * (l >> 4):16 * d8 + 4 * (l >> 4) + 4] = blk[l]
    assert np.array_equal(out, (Vt @ ST).T)  # O = P V with P = S


def test_fragment_reads_are_free_of_bank_conflicts():
    def slots(addr_fn):
        for grp in B128_GROUPS:
            s = [(addr_fn(l) * 2 // 16) % 16 for l in grp]
            assert len(set(s)) == 16, s
    for ks in range(4):
        for kb in range(4):
            slots(lambda l: k_frag_addr(l, ks, kb))
    for G in range(2):
        for d8 in range(8):
            slots(lambda l: v_frag_addr(l, G, d8))
    # with the w4b kernel's swizzle (chunk ^ (row & 15)) the same K fragment read would be 2-way: the reason the kernel has its own
    w4b = lambda l: (8 * ((l & 15) >> 2) + ((l & 15) & 3)) * HD + (((l >> 4) ^ ((8 * ((l & 15) >> 2) + ((l & 15) & 3)) & 15)) << 3)
    assert max(len(grp) - len({(w4b(l) * 2 // 16) % 16 for l in grp}) for grp in B128_GROUPS) == 8
