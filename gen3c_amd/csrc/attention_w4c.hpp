// Included by attention.hip after attention_w4b.hpp, inside the same anonymous namespace: flash_attn_fwd_w4c_nm_kernel, the no-max one-wave-per-SIMD
// self-attention kernel (attention_w4b.hpp, NM + XB form) with its tile loop on v_mfma_f32_16x16x32_bf16 instead of v_mfma_f32_32x32x16_bf16.
// Why: the tile loop is limited by the clock the chip holds under load, not by issue slots, and it holds a higher clock on the 16x16x32 shape
// (tools/mfma_shape_probe.hip, profiles/mfma_shape_probe.txt: 2592 instead of 2363 cycles per tile at 1.81 instead of 1.60 GHz, +6.4 % by wall).
// Only the form the DiT step launches: bounded logits (AttnParams::logit_bound_log2), plain V^T, no carry / skip / segments, no kv_dense, bf16
// output, no Q norm, S_kv % 64 == 0 (g3_self_attn_fwd_bounded16_bf16; every other call runs the kernel it always ran).
// Same structure as w4b: 256 query rows per workgroup, a wave owns 64 query columns of S^T = K Q^T, K / V^T tiles of 64 keys by LDS-DMA into two
// stages each (64 KiB), O^T in a[0:127], Q in a[128:191], a 16-slot fragment ring in a[192:255] read W4C_D groups ahead (across the tile barrier
// into the next tile's K), the XCD-local (batch, head) walk, P rounded to bf16, row sums and O in fp32.
// What the shape changes:
//   * a GROUP is one fragment and the four MFMAs it feeds (the wave's four 16-query blocks): 16 K groups (region A: key block kb = I & 3, k-step of 32
//     dims ks = I >> 2) and 16 V^T groups (region B: 32-key group G = I >> 3, 16-dim output block d8 = I & 7) per tile, one ds_read_b128 each.
//   * D of a 16x16x32 block: lane l holds query l & 15, rows 4 (l >> 4) + r. The P.V B operand wants keys 8 (l >> 4) .. + 7 of a 32-key group per
//     lane. Row 4 g + r of key block b = kb & 1 of group G = kb >> 1 therefore loads physical key 32 G + 8 g + 4 b + r: the two blocks' D registers
//     of a lane are then exactly its eight keys, in order, V^T stays in natural key order and P needs no cross-lane move
//     (tests/test_attn_w4c_layout_cpu.py proves the composition).
//   * the K tile's LDS swizzle is this kernel's own: chunk c of row `row` sits at chunk c ^ w4c_kswz(row), w4c_kswz = (row & 3) | ((row >> 3) & 3) << 2,
//     which takes the 16 rows of one fragment to 16 different values: the ds_read_b128 of a fragment is conflict-free (with w4b's row & 15 it would be
//     2-way: the rows of a fragment share bit 2). Linear LDS-DMA destination, permuted source chunk, permuted read - all three in this file.
//     V^T keeps w4b's layout (its 16x16x32 fragment read is conflict-free as it is).
//   * schedule: region A group = [m0] read wait QK exp QK exp [piece] QK add add QK cvt (pair units 0..15, the four V^T(t+1) LDS-DMA pieces on groups 8, 10,
//     12, 14); region B groups 0..7 carry two pair units each (16..31, needed from group 8 on), groups 8..15 none; the barrier sits in front of group 10.
//     No statement reads a transcendental's result in the next instruction.
//   * K is fetched one tile ahead, behind the barrier: the four K(t+3) pieces sit in four bare groups >= 10 of region B of tile t and land in the stage of
//     K(t+1), which region A of tile t has finished with. A piece there shares its group with four MFMAs only, not with a pair unit. K(2) comes from the
//     prologue; the tail fetches the last tile again; one vmcnt(0) in front of the epilogue drains what the last tiles left in flight.
constexpr int W4C_D = 6;  // fragment n is read W4C_D groups before the group that consumes it
constexpr int W4C_KG0 = 12;  // region-B groups W4C_KG0 .. + 3 carry the K pieces (tools/mfma_shape_probe.hip: arms (K10) and (K12) tie; 12..15 had the steadier runs)
static_assert(W4C_KG0 >= 10 && W4C_KG0 + 4 <= 16, "the K pieces overwrite K(t+1)'s stage: only behind the barrier in front of group 10");

// MIRRORED in tests/test_attn_w4c_layout_cpu.py (kswz, k_off, lds_dma_images = dma_off below, k_frag_addr = kaddr, v_frag_addr = vaddr): the host model
// proves the layout from hand copies of these formulas, so an edit to w4c_kswz, w4c_k_off, dma_off, kaddr or vaddr must be made there as well.

G3_DEVICE int w4c_kswz(int row) { return (row & 3) | (((row >> 3) & 3) << 2); }
G3_DEVICE int w4c_k_off(int row, int chunk) { return row * HD + ((chunk ^ w4c_kswz(row)) << 3); }  // [64][128]

#if G3_AB_ATTN_ABLATE & 32
#define W4C_READ ""
#else
#define W4C_READ "ds_read_b128 a[%c[ra]:%c[ra]+3], %[addr] offset:%c[off]\n\t"
#endif
#define W4C_QK(h) "v_mfma_f32_16x16x32_bf16 %[s" #h "], a[%c[fa]:%c[fa]+3], a[%c[q" #h "]:%c[q" #h "]+3], %[s" #h "]\n\t"
#define W4C_QK0(h) "v_mfma_f32_16x16x32_bf16 %[s" #h "], a[%c[fa]:%c[fa]+3], a[%c[q" #h "]:%c[q" #h "]+3], %[c]\n\t"
#define W4C_PV(h) "v_mfma_f32_16x16x32_bf16 a[%c[o" #h "]:%c[o" #h "]+3], a[%c[fa]:%c[fa]+3], %[pf" #h "], a[%c[o" #h "]:%c[o" #h "]+3]\n\t"
#if G3_AB_ATTN_ABLATE & 16
#define W4C_EXPA(n) "v_mov_b32 %[k" #n "], 0\n\t"
#define W4C_EXPB(n) ""
#define W4C_ADDS(n) ""
#define W4C_CVT(n) ""
#else
#define W4C_EXPA(n) "v_exp_f32 %[a" #n "], %[x" #n "]\n\t"
#define W4C_EXPB(n) "v_exp_f32 %[b" #n "], %[y" #n "]\n\t"
#define W4C_ADDS(n) "v_add_f32 %[p" #n "], %[p" #n "], %[a" #n "]\n\tv_add_f32 %[r" #n "], %[r" #n "], %[b" #n "]\n\t"
#define W4C_CVT(n) "v_cvt_pk_bf16_f32 %[k" #n "], %[a" #n "], %[b" #n "]\n\t"
#endif
#define W4C_UNIT_OUT(n, u) [a##n] "+v"(u.a), [b##n] "+v"(u.b), [k##n] "=&v"(u.k), [p##n] "+v"(u.p), [r##n] "+v"(u.r)
#define W4C_UNIT_IN(n, u) [x##n] "v"(u.x), [y##n] "v"(u.y)

struct W4cUnit {  // one pair unit: scores x, y in; exp2 temporaries a, b; the two row-sum accumulators p, r; the packed P dword k out
    float x, y;
    float &a, &b, &p, &r;
    uint32_t k;
};

// ---- region A group I: [m0] read wait ; S(q0) (+)= K.Q0 ; exp ; S(q1) ; exp ; [LDS-DMA piece] ; S(q2) ; add add ; S(q3) ; cvt
template <int I, int ROFF, bool DMA>
G3_DEVICE void w4c_group_qk(uint32_t addr, f32x4& s0, f32x4& s1, f32x4& s2, f32x4& s3, const f32x4& c, W4cUnit& u1, uint32_t m0v, uint32_t voff, const char* sbase) {
    constexpr int ks = I >> 2, q0 = W4_QBASE + 4 * ks, q1 = q0 + 16, q2 = q0 + 32, q3 = q0 + 48;  // Q fragment (qb, ks) in a[128 + 4 (4 qb + ks) : +3]
    constexpr int fa = W4B_RING0 + 4 * (I & 15), ra = W4B_RING0 + 4 * ((I + W4C_D) & 15);
#define W4C_A_IN [addr] "v"(addr), [off] "n"(ROFF), [wn] "n"(W4C_D), [fa] "n"(fa), [ra] "n"(ra), W4C_UNIT_IN(1, u1), [q0] "n"(q0), [q1] "n"(q1), [q2] "n"(q2), [q3] "n"(q3)
    if constexpr (ks == 0 && DMA)
        asm volatile(W4B_M0 W4C_READ W4_WAIT W4C_QK0(0) W4C_EXPA(1) W4C_QK0(1) W4C_EXPB(1) W4B_DMA W4C_QK0(2) W4C_ADDS(1) W4C_QK0(3) W4C_CVT(1)
                     : W4C_UNIT_OUT(1, u1), [s0] "=&v"(s0), [s1] "=&v"(s1), [s2] "=&v"(s2), [s3] "=&v"(s3)
                     : W4C_A_IN, [c] "v"(c), [m0v] "s"(m0v), [voff] "v"(voff), [sbase] "s"(sbase) : "memory");
    else if constexpr (ks == 0)
        asm volatile(W4C_READ W4_WAIT W4C_QK0(0) W4C_EXPA(1) W4C_QK0(1) W4C_EXPB(1) W4C_QK0(2) W4C_ADDS(1) W4C_QK0(3) W4C_CVT(1)
                     : W4C_UNIT_OUT(1, u1), [s0] "=&v"(s0), [s1] "=&v"(s1), [s2] "=&v"(s2), [s3] "=&v"(s3) : W4C_A_IN, [c] "v"(c));
    else if constexpr (DMA)
        asm volatile(W4B_M0 W4C_READ W4_WAIT W4C_QK(0) W4C_EXPA(1) W4C_QK(1) W4C_EXPB(1) W4B_DMA W4C_QK(2) W4C_ADDS(1) W4C_QK(3) W4C_CVT(1)
                     : W4C_UNIT_OUT(1, u1), [s0] "+v"(s0), [s1] "+v"(s1), [s2] "+v"(s2), [s3] "+v"(s3)
                     : W4C_A_IN, [m0v] "s"(m0v), [voff] "v"(voff), [sbase] "s"(sbase) : "memory");
    else
        asm volatile(W4C_READ W4_WAIT W4C_QK(0) W4C_EXPA(1) W4C_QK(1) W4C_EXPB(1) W4C_QK(2) W4C_ADDS(1) W4C_QK(3) W4C_CVT(1)
                     : W4C_UNIT_OUT(1, u1), [s0] "+v"(s0), [s1] "+v"(s1), [s2] "+v"(s2), [s3] "+v"(s3) : W4C_A_IN);
#undef W4C_A_IN
}

// ---- region B group I: [read] wait ; O(d8, q0) += V^T.P0 ; [exp exp] ; O(d8, q1) ; [add add cvt] ; O(d8, q2) ; [exp exp] ; O(d8, q3) ; [add add cvt]
//      DMA form (a bare group behind the barrier): [m0] read wait ; O(d8, q0) ; O(d8, q1) ; LDS-DMA piece ; O(d8, q2) ; O(d8, q3)
template <int I, int ROFF, bool READ, int WN, bool UNITS, bool DMA>
G3_DEVICE void w4c_group_pv(uint32_t addr, const u32x4& pf0, const u32x4& pf1, const u32x4& pf2, const u32x4& pf3, W4cUnit& u1, W4cUnit& u2, uint32_t m0v, uint32_t voff,
                            const char* sbase) {
    constexpr int o0 = 16 * (I & 7), o1 = o0 + 4, o2 = o0 + 8, o3 = o0 + 12;  // O^T block (d8, qb) in a[4 (4 d8 + qb) : +3]
    constexpr int fa = W4B_RING0 + 4 * ((16 + I) & 15), ra = W4B_RING0 + 4 * ((16 + I + W4C_D) & 15);
#define W4C_B_IN [pf0] "v"(pf0), [pf1] "v"(pf1), [pf2] "v"(pf2), [pf3] "v"(pf3), [wn] "n"(WN), [fa] "n"(fa), [o0] "n"(o0), [o1] "n"(o1), [o2] "n"(o2), [o3] "n"(o3)
#define W4C_B_RD [addr] "v"(addr), [off] "n"(ROFF), [ra] "n"(ra)
    static_assert(!UNITS || READ, "the groups with pair units (0..7) always read ahead");
    static_assert(!DMA || (READ && !UNITS), "a piece sits in a bare group of a tile that has a next one");
    if constexpr (DMA)
        asm volatile(W4B_M0 W4C_READ W4_WAIT W4C_PV(0) W4C_PV(1) W4B_DMA W4C_PV(2) W4C_PV(3)
                     : : W4C_B_IN, W4C_B_RD, [m0v] "s"(m0v), [voff] "v"(voff), [sbase] "s"(sbase) : "memory");
    else if constexpr (UNITS)
        asm volatile(W4C_READ W4_WAIT W4C_PV(0) W4C_EXPA(1) W4C_EXPB(1) W4C_PV(1) W4C_ADDS(1) W4C_CVT(1) W4C_PV(2) W4C_EXPA(2) W4C_EXPB(2) W4C_PV(3) W4C_ADDS(2) W4C_CVT(2)
                     : W4C_UNIT_OUT(1, u1), W4C_UNIT_OUT(2, u2) : W4C_B_IN, W4C_B_RD, W4C_UNIT_IN(1, u1), W4C_UNIT_IN(2, u2));
    else if constexpr (READ)
        asm volatile(W4C_READ W4_WAIT W4C_PV(0) W4C_PV(1) W4C_PV(2) W4C_PV(3) : : W4C_B_IN, W4C_B_RD);
    else
        asm volatile(W4_WAIT W4C_PV(0) W4C_PV(1) W4C_PV(2) W4C_PV(3) : : W4C_B_IN);
#undef W4C_B_IN
#undef W4C_B_RD
}

// the first W4C_D fragments of a tile (ring slots 0..5) outside a group, one statement
template <int O0, int O1, int O2, int O3, int O4, int O5> G3_DEVICE void w4c_read_head(uint32_t ad0, uint32_t ad1, uint32_t ad2, uint32_t ad3, uint32_t ad4, uint32_t ad5) {
    static_assert(W4C_D == 6, "w4c_read_head is laid out for a read-ahead of 6");
    if (!(G3_AB_ATTN_ABLATE & 32))
        asm volatile("ds_read_b128 a[192:195], %0 offset:%c6\n\tds_read_b128 a[196:199], %1 offset:%c7\n\tds_read_b128 a[200:203], %2 offset:%c8\n\t"
                     "ds_read_b128 a[204:207], %3 offset:%c9\n\tds_read_b128 a[208:211], %4 offset:%c10\n\tds_read_b128 a[212:215], %5 offset:%c11"
                     ::"v"(ad0), "v"(ad1), "v"(ad2), "v"(ad3), "v"(ad4), "v"(ad5), "n"(O0), "n"(O1), "n"(O2), "n"(O3), "n"(O4), "n"(O5) : W4B_OWNED);
}

// prologue only: S block (+)= K fragment (compiler-managed read) . Q fragment (qb, ks)
template <int QF> G3_DEVICE void w4c_qk_c(f32x4& S, const bf16x8& kfrag) {
    asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, a[%c2:%c2+3], %0" : "+v"(S) : "v"(kfrag), "n"(W4_QBASE + 4 * QF) : W4B_OWNED);
}
// 4-pass MFMA results in VGPRs -> first VALU reader: wait states, tied to the registers so that no reader is scheduled above the fence
G3_DEVICE void w4c_fence_v(f32x4& a, f32x4& b, f32x4& c, f32x4& d) { asm volatile("s_nop 7\n\ts_nop 3" : "+v"(a), "+v"(b), "+v"(c), "+v"(d)); }

__global__ __launch_bounds__(W4_THREADS, 1) void flash_attn_fwd_w4c_nm_kernel(AttnParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    bf16_t* sK = reinterpret_cast<bf16_t*>(smem_raw);  // [2][64][128]
    bf16_t* sV = sK + 2 * KVB * HD;                     // [2][128][64]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15;
    const int g = lane >> 4;
    int qblk = blockIdx.x, head = blockIdx.y, batch = blockIdx.z;
    if (p.xcd_heads) {  // 1-D grid: XCD x (= workgroup index % 8) works through the (batch, head) pairs x, x + 8, x + 16, ... (as w4b)
        const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
        const int hb = xcd + 8 * (slot / p.grid_q);
        qblk = slot - (slot / p.grid_q) * p.grid_q;
        head = hb % p.n_heads;
        batch = hb / p.n_heads;
    }
    const bf16_t* Qb = p.Q + batch * p.q_batch + head * p.q_head;
    const bf16_t* Kb = p.K + batch * p.k_batch + head * p.k_head;
    const bf16_t* Vb = p.Vt + batch * p.vt_batch + head * p.vt_head;
    bf16_t* Ob = p.O + batch * p.o_batch + head * p.o_head;
    // fetched from the kernel arguments HERE (opaque to the optimiser), not by a scalar load near the tile loop, whose lgkmcnt waits are hand-counted
    float bound = p.logit_bound_log2;
    asm volatile("" : "+s"(bound));

    // ---- Q fragments (qb, ks), pre-multiplied by scale * log2(e), into a[128:191]: lane = query 16 qb + l15, dims 32 ks + 8 g .. + 7; O accumulators = 0
    static_for<0, 16>([&](auto fc) {
        constexpr int f = decltype(fc)::value, qb = f >> 2, ks = f & 3;
        const int q_idx = qblk * W4_BQ + wave * 64 + 16 * qb + l15;
        bf16x8 qv = q_idx < p.Sq ? load_bf16x8(Qb + (int64_t)q_idx * p.q_row + 32 * ks + 8 * g) : zero_bf16x8();
#pragma unroll
        for (int e = 0; e < 8; ++e) qv[e] = f32_to_bf16((float)qv[e] * p.scale_log2);
        const u32x4 qw = __builtin_bit_cast(u32x4, qv);
        w4_acc_write<W4_QBASE + 4 * f + 0>(qw[0]);
        w4_acc_write<W4_QBASE + 4 * f + 1>(qw[1]);
        w4_acc_write<W4_QBASE + 4 * f + 2>(qw[2]);
        w4_acc_write<W4_QBASE + 4 * f + 3>(qw[3]);
    });
    static_for<0, 128>([&](auto rc) { w4_acc_zero<decltype(rc)::value>(); });

    // ---- LDS-DMA staging: w4b's slots and V^T source; the K source chunk follows this kernel's swizzle
    const int k_row0 = tid >> 4, v_row0 = tid >> 3, v_src_chunk = (tid & 7) ^ ((v_row0 >> 1) & 7);
    const char* Kbytes = reinterpret_cast<const char*>(Kb);
    const char* Vbytes = reinterpret_cast<const char*>(Vb);
    const uint32_t k_row_bytes = (uint32_t)p.k_row * 2u;
    const uint32_t v_row_bytes = (uint32_t)p.vt_row * 2u;
    uint32_t dma_off[8];  // [0..3] K piece j (rows k_row0 + 16 j of the tile), [4..7] V^T piece j (rows v_row0 + 32 j)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        dma_off[j] = ((uint32_t)k_row0 + 16u * j) * k_row_bytes + (uint32_t)((tid & 15) ^ w4c_kswz(k_row0 + 16 * j)) * 16u;
        dma_off[4 + j] = ((uint32_t)v_row0 + 32u * j) * v_row_bytes + (uint32_t)v_src_chunk * 16u;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) asm volatile("" : "+v"(dma_off[j]));  // opaque: keep them resident instead of re-deriving them per piece
    const uint32_t k_tile_bytes = (uint32_t)KVB * k_row_bytes;
    auto dma_tile_builtin = [&](const char* base, const uint32_t* off, bf16_t* dst) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(base + off[i]),
                                             (__attribute__((address_space(3))) void*)(dst + wave * 64 * 8 + 256 * 8 * i), 16, 0, 0);
    };

    // ---- per-lane LDS byte addresses of the fragments inside stage 0: K (k-step ks, key block parity b): A row l15 = physical key 8 (l15 >> 2) + 4 b + (l15 & 3)
    // of the 32-key group, dims chunk 4 ks + g; V^T (key group G): A row l15 = output dim l15 of the block, keys chunk 4 G + g
    const uint32_t lds_k0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) bf16_t*)sK;
    const uint32_t lds_v0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) bf16_t*)sV;
    const int krow = 8 * (l15 >> 2) + (l15 & 3);
    uint32_t kaddr[4][2], vaddr[2];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int b = 0; b < 2; ++b) kaddr[ks][b] = lds_k0 + 2u * (uint32_t)w4c_k_off(krow + 4 * b, 4 * ks + g);
#pragma unroll
    for (int G = 0; G < 2; ++G) vaddr[G] = lds_v0 + 2u * (uint32_t)v_off(l15, 4 * G + g);

    // row sums: [query block][step parity x lane of the pair] - consecutive statements of region A never name the same one
    float psum[4][4];
#pragma unroll
    for (int qb = 0; qb < 4; ++qb)
#pragma unroll
        for (int k = 0; k < 4; ++k) psum[qb][k] = 0.f;
    float ta[2] = {0.f, 0.f}, tb[2] = {0.f, 0.f};  // exp2 results of a pair unit, one set per parity
    const int nt = p.Skv / KVB;                     // launcher: S_kv % 64 == 0

    // ---- prologue: K(0), V(0) (and K(1)) by LDS-DMA; scores of tile 0 with C = 0, then made relative to the bound (as w4b's no-max form)
    dma_tile_builtin(Kbytes, dma_off, sK);
    dma_tile_builtin(Vbytes, dma_off + 4, sV);
    if (nt > 1) dma_tile_builtin(Kbytes + k_tile_bytes, dma_off, sK + KVB * HD);
    G3_JITTER(wave, blockIdx.x + 5);
    lds_dma_publish_barrier();
    G3_JITTER(wave + 2, blockIdx.x);
    f32x4 SA[4][4], SB[4][4];  // [16-key block kb][query block qb]
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int qb = 0; qb < 4; ++qb) SA[kb][qb] = f32x4{0.f, 0.f, 0.f, 0.f};
    static_for<0, 16>([&](auto ic) {
        constexpr int i = decltype(ic)::value, kb = i >> 2, ks = i & 3;
        const bf16x8 kf = load_bf16x8(sK + w4c_k_off(32 * (kb >> 1) + krow + 4 * (kb & 1), 4 * ks + g));  // compiler-managed read + wait (prologue only)
        w4c_qk_c<ks>(SA[kb][0], kf);
        w4c_qk_c<4 + ks>(SA[kb][1], kf);
        w4c_qk_c<8 + ks>(SA[kb][2], kf);
        w4c_qk_c<12 + ks>(SA[kb][3], kf);
    });
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) w4c_fence_v(SA[kb][0], SA[kb][1], SA[kb][2], SA[kb][3]);
    __syncthreads();  // K(0)'s slot is the destination of the next LDS-DMA (K(2)): every wave must be done reading it
    // K runs one tile ahead of the loop's own fetches (tile t fetches K(t+3) behind its barrier): K(2) from here, drained and published by tile 0's barrier
    if (nt > 2) dma_tile_builtin(Kbytes + 2u * k_tile_bytes, dma_off, sK);
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int qb = 0; qb < 4; ++qb)
#pragma unroll
            for (int r = 0; r < 4; ++r) SA[kb][qb][r] -= bound;
    f32x4 negm = f32x4{-bound, -bound, -bound, -bound};  // C operand of the first QK^T MFMA of a block
    asm volatile("" : "+v"(negm));                        // resident VGPRs, not SGPR copies per tile
    if (nt > 1) {  // the first six K(1) fragments (stage 1, published by the prologue barrier): tile 0 starts with them in the ring
        constexpr int KS1 = KVB * HD * 2;
        w4c_read_head<KS1, KS1, KS1 + 8192, KS1 + 8192, KS1, KS1>(kaddr[0][0], kaddr[0][1], kaddr[0][0], kaddr[0][1], kaddr[1][0], kaddr[1][1]);
    }
    uint32_t v_off_next = (uint32_t)(KVB * 2);  // byte offset of V^T tile t + 1 inside a V^T row

    auto tile = [&](f32x4 (&S_cur)[4][4], f32x4 (&S_next)[4][4], int t, auto has_next_c, auto par_c) {
        constexpr bool has_next = decltype(has_next_c)::value;
        constexpr int par = decltype(par_c)::value;
        constexpr int D = W4C_D;
        constexpr int KS = (par ^ 1) * KVB * HD * 2;  // LDS byte offset of K(t+1)'s stage
        constexpr int VS = par * HD * KVB * 2;         // of V^T(t)'s stage
        constexpr int KSN = par * KVB * HD * 2;        // of K(t+2)'s stage (read across the barrier)
        // fragment n: K fragments 0..15 (group n: kb = n & 3, ks = n >> 2), V^T fragments 16..31 (group n - 16: G = (n - 16) >> 3, d8 = (n - 16) & 7), 32..: the
        // next tile's K fragments. Byte offset (immediate) and per-lane address register.
        auto frag_off = [](auto nc) constexpr {
            constexpr int n = decltype(nc)::value;
            return n < 16 ? KS + 8192 * ((n & 3) >> 1) : n < 32 ? VS + 2048 * ((n - 16) & 7) : KSN + 8192 * (((n - 32) & 3) >> 1);
        };
        auto frag_addr = [&](auto nc) -> uint32_t {
            constexpr int n = decltype(nc)::value;
            if constexpr (n < 16) return kaddr[n >> 2][n & 1];
            else if constexpr (n < 32) return vaddr[(n - 16) >> 3];
            else return kaddr[(n - 32) >> 2][(n - 32) & 1];
        };
        G3_JITTER(wave + blockIdx.x, t);  // race screen only
        if constexpr (!has_next) {  // the last tile has no region A: its first six V^T fragments are read here
            using N0 = std::integral_constant<int, 16>;
            using N1 = std::integral_constant<int, 17>;
            using N2 = std::integral_constant<int, 18>;
            using N3 = std::integral_constant<int, 19>;
            using N4 = std::integral_constant<int, 20>;
            using N5 = std::integral_constant<int, 21>;
            w4c_read_head<frag_off(N0{}), frag_off(N1{}), frag_off(N2{}), frag_off(N3{}), frag_off(N4{}), frag_off(N5{})>(vaddr[0], vaddr[0], vaddr[0], vaddr[0], vaddr[0], vaddr[0]);
        }
        u32x4 pb[2][4];  // P fragments (bf16 pairs): key group G, query block qb; dword 2 b + pr = keys 8 g + 4 b + 2 pr, + 1
        // pair unit u = 0..31 in consumption order: key group G = u >> 4, query block qb = (u >> 2) & 3, key block parity b = (u >> 1) & 1, pair pr = u & 1
        auto ux = [&](auto uc) -> float { constexpr int u = decltype(uc)::value; return S_cur[2 * (u >> 4) + ((u >> 1) & 1)][(u >> 2) & 3][2 * (u & 1)]; };
        auto uy = [&](auto uc) -> float { constexpr int u = decltype(uc)::value; return S_cur[2 * (u >> 4) + ((u >> 1) & 1)][(u >> 2) & 3][2 * (u & 1) + 1]; };
        auto uput = [&](auto uc, uint32_t pk) { constexpr int u = decltype(uc)::value; pb[u >> 4][(u >> 2) & 3][2 * ((u >> 1) & 1) + (u & 1)] = pk; };
        if constexpr (!has_next) {  // pair units 0..15 outside a group
            static_for<0, 16>([&](auto uc) {
                constexpr int u = decltype(uc)::value, qb = (u >> 2) & 3, pa = 2 * (u & 1);
                float a, b;
                uint32_t pk;
                if (G3_AB_ATTN_ABLATE & 16) {
                    pk = 0;
                } else {
                    asm volatile("v_exp_f32 %0, %5\n\tv_exp_f32 %1, %6\n\tv_add_f32 %3, %3, %0\n\tv_add_f32 %4, %4, %1\n\tv_cvt_pk_bf16_f32 %2, %0, %1"
                                 : "=&v"(a), "=&v"(b), "=v"(pk), "+v"(psum[qb][pa]), "+v"(psum[qb][pa + 1]) : "v"(ux(uc)), "v"(uy(uc)));
                }
                uput(uc, pk);
            });
        }
        // ---- region A: S_next = K(t+1).Q^T; pair unit I; the V^T(t+1) LDS-DMA pieces 0..3 on groups 8, 10, 12, 14 -> stage of V^T(t-1) (as w4b). The K pieces
        //      are not here: a piece beside a pair unit costs the group issue cycles, and K can be fetched in the bare groups of region B (below)
        if constexpr (has_next) {
            const char* vbase = Vbytes + v_off_next;
            static_for<0, 16>([&](auto ic) {
                constexpr int I = decltype(ic)::value, kb = I & 3, qb = (I >> 2) & 3, pa = 2 * (I & 1);
                using NR = std::integral_constant<int, I + D>;
                using U = std::integral_constant<int, I>;
                constexpr bool dma = I >= 8 && (I & 1) == 0;
                constexpr int j = dma ? (I - 8) >> 1 : 0;
                const uint32_t m0v = dma ? lds_v0 + (uint32_t)((par ^ 1) * HD * KVB * 2 + 256 * j * 16) + (uint32_t)wave * 1024u : 0u;
                W4cUnit u1{ux(U{}), uy(U{}), ta[I & 1], tb[I & 1], psum[qb][pa], psum[qb][pa + 1], 0u};
                w4c_group_qk<I, frag_off(NR{}), dma>(frag_addr(NR{}), S_next[kb][0], S_next[kb][1], S_next[kb][2], S_next[kb][3], negm, u1, m0v, dma_off[4 + j], vbase);
                uput(U{}, u1.k);
            });
            v_off_next += (uint32_t)(KVB * 2);
        }
        G3_JITTER(wave + blockIdx.x + 3, t);
        // K one tile ahead: K(t+3) pieces 0..3 in the bare groups W4C_KG0 .. + 3 of region B, behind the barrier, into the stage of K(t+1). That stage is read in
        // region A of this tile only; a wave waits for its last K(t+1) fragment in group 15 of region A and LDS returns reads in order, so every wave that has
        // arrived at the barrier is done with it. The pieces have a whole tile of lead; tile t + 1's vmcnt(0) + barrier drains and publishes them together with
        // that tile's V^T pieces. Past the end the last tile is fetched again (in bounds; nobody consumes the stage any more).
        const char* kbase = Kbytes + (uint32_t)min(t + 3, nt - 1) * k_tile_bytes;
        // ---- region B: O^T += V^T(t).P^T, group I: key group G = I >> 3, output block d8 = I & 7; pair units 16 + 2 I, 17 + 2 I in groups 0..7
        static_for<0, 16>([&](auto ic) {
            constexpr int I = decltype(ic)::value, G = I >> 3;
            constexpr bool rd = (I + D < 16) || has_next;
            constexpr bool units = I < 8;
            using NR = std::integral_constant<int, rd ? 16 + I + D : 16>;
            using U1 = std::integral_constant<int, units ? 16 + 2 * I : 16>;
            using U2 = std::integral_constant<int, units ? 17 + 2 * I : 17>;
            constexpr int qb = (U1::value >> 2) & 3;
            if constexpr (has_next && I == 10) {
                // every wave has issued its last read of V^T(t) (group 9) and of K(t+1) (region A): drain this wave's LDS-DMA and publish K(t+2) / V^T(t+1).
                // No operands: the statement shares no register with its neighbours (no pad).
                if (!(G3_AB_ATTN_ABLATE & 64)) asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
                G3_JITTER(wave + blockIdx.x + 1, t);  // race screen only: between the barrier and the first piece into the stage the barrier has freed
            }
            constexpr bool dma = has_next && I >= W4C_KG0 && I < W4C_KG0 + 4;
            constexpr int j = dma ? I - W4C_KG0 : 0;
            const uint32_t m0v = dma ? lds_k0 + (uint32_t)((par ^ 1) * KVB * HD * 2 + 256 * j * 16) + (uint32_t)wave * 1024u : 0u;
            W4cUnit u1{ux(U1{}), uy(U1{}), ta[0], tb[0], psum[qb][0], psum[qb][1], 0u};
            W4cUnit u2{ux(U2{}), uy(U2{}), ta[1], tb[1], psum[qb][2], psum[qb][3], 0u};
            w4c_group_pv<I, frag_off(NR{}), rd, rd ? D : 15 - I, units, dma>(frag_addr(NR{}), pb[G][0], pb[G][1], pb[G][2], pb[G][3], u1, u2, m0v, dma_off[j], kbase);
            if constexpr (units) {
                uput(U1{}, u1.k);
                uput(U2{}, u2.k);
            }
        });
    };

    using True = std::integral_constant<bool, true>;
    using False = std::integral_constant<bool, false>;
    using P0 = std::integral_constant<int, 0>;
    using P1 = std::integral_constant<int, 1>;
    int t = 0;
    for (; t + 2 < nt; t += 2) {
        tile(SA, SB, t, True{}, P0{});
        tile(SB, SA, t + 1, True{}, P1{});
    }
    if (t + 1 < nt) {
        tile(SA, SB, t, True{}, P0{});
        tile(SB, SA, t + 1, False{}, P1{});
    } else {
        tile(SA, SB, t, False{}, P0{});
    }

    // The last tile has no barrier and so no vmcnt(0): the pieces that tile nt - 2 issued behind its barrier (a re-fetch of the last K tile, which nobody
    // reads) may still be in flight. Each wave waits for its own here, so no LDS-DMA write can land after the workgroup has given its LDS back (a workgroup's
    // LDS is released when its last wave ends, and a wave's pieces are counted in that wave's vmcnt alone).
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // ---- epilogue: a query's row sum is spread over the four lanes l15 + 16 g; O^T block (d8, qb) register r = output dim 16 d8 + 4 g + r of query 16 qb + l15
    w4b_fence_acc();
    static_for<0, 4>([&](auto qc) {
        constexpr int qb = decltype(qc)::value;
        float l = (psum[qb][0] + psum[qb][1]) + (psum[qb][2] + psum[qb][3]);
        l += __shfl_xor(l, 16);
        l += __shfl_xor(l, 32);
        const float inv = 1.0f / l;
        const int q_idx = qblk * W4_BQ + wave * 64 + 16 * qb + l15;
        bf16_t* orow = Ob + (int64_t)q_idx * p.o_row;
        static_for<0, 8>([&](auto dc) {
            constexpr int d8 = decltype(dc)::value;
            constexpr int R = 4 * (4 * d8 + qb);
            bf16x4 o;
            o[0] = f32_to_bf16(w4_acc_read<R + 0>() * inv);
            o[1] = f32_to_bf16(w4_acc_read<R + 1>() * inv);
            o[2] = f32_to_bf16(w4_acc_read<R + 2>() * inv);
            o[3] = f32_to_bf16(w4_acc_read<R + 3>() * inv);
            if (q_idx < p.Sq) *reinterpret_cast<bf16x4*>(orow + 16 * d8 + 4 * g) = o;
        });
    });
}
