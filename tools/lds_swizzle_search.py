"""Exhaustive bank-conflict check / search of the k_conv_stream LDS images for the v_mfma_f32_16x16x32_bf16
operand layout (lane l reads row l & 15, 16-B k-group l >> 4 with one ds_read_b128).

ds_read_b128 serves a wave in four 16-lane groups (MI355X_MICROARCH.md, LDS table); a group is conflict-free
when its 16 lanes hit 16 distinct 16-B bank units of a 256-B line.  Checked for every tap offset and for the
three tile geometries of conv_stream.hip (5x5 16x16, 3x3 16x16, 3x3 8x8 x 4 clips).

The split-f16 planar slice pairs read other lane -> slot maps from the same images: every lane takes 16-B slot kg & 1
(h halves) or 2 + (kg & 1) (l halves), and lanes 32..63 read the pair's second slice (another tap, possibly another
halo slot, and the next weight ring slot: whole multiples of 1 KB away).  A 16-lane service group never spans both
halves of the wave, so a group sees one tap and one slot; the maps are checked below over every tap like the bf16 one.
    python tools/lds_swizzle_search.py
"""
import itertools

GROUPS = [[0, 1, 2, 3, 12, 13, 14, 15] + list(range(20, 28)), list(range(4, 12)) + [16, 17, 18, 19, 28, 29, 30, 31]]
GROUPS += [[g + 32 for g in grp] for grp in GROUPS]
GEOMS = [dict(KS=5, TH=16, TW=16, NC=1), dict(KS=3, TH=16, TW=16, NC=1), dict(KS=3, TH=8, TW=8, NC=4)]


def lane_pixel(lane):
    """Row r = 4 q + 2 dy + dx of a 4x4-pixel block -> pixel (2 (q >> 1) + dy, 2 (q & 1) + dx); k-group."""
    r, k = lane & 15, lane >> 4
    q, dy, dx = r >> 2, (r >> 1) & 1, r & 1
    return 2 * (q >> 1) + dy, 2 * (q & 1) + dx, k


# lane -> 16-B slot (before the image's xor): the bf16 / swap-form operand layout, and the planar slice pairs' two halves
KMAPS = {"bf16": lambda lane: lane >> 4, "planar h": lambda lane: (lane >> 4) & 1,
         "planar l": lambda lane: 2 + ((lane >> 4) & 1)}


def halo_ok(f, kmap=KMAPS["bf16"]):
    for g in GEOMS:
        ks = g["KS"]
        hh, hw = g["TH"] + ks - 1, g["TW"] + ks - 1
        for cl in range(g["NC"]):
            for y0 in range(0, g["TH"], 4):
                for x0 in range(0, g["TW"], 4):
                    for ky in range(ks):
                        for kx in range(ks):
                            for grp in GROUPS:
                                units = set()
                                for lane in grp:
                                    py, px, _ = lane_pixel(lane)
                                    y, x = y0 + py + ky, x0 + px + kx
                                    p = (cl * hh + y) * hw + x
                                    units.add((4 * (p % 4) + (kmap(lane) ^ f(y))) % 16)
                                if len(units) < 16:
                                    return False
    return True


def weights_ok(tab, kmap=KMAPS["bf16"]):
    for jb in range(8):
        for grp in GROUPS:
            units = {(4 * ((16 * jb + (l & 15)) % 4) + (kmap(l) ^ tab[((16 * jb + (l & 15)) >> 2) & 3])) % 16 for l in grp}
            if len(units) < 16:
                return False
    return True


def v1r_read2_cycles(pitch, pb=12):
    """conv_v1r.hip A fragments: lane (r16, kg) reads 16 B at window pixel (y, x) of its 4x4 block, byte
    16 kg, as 4 dwords (two ds_read2_b32); ds_read_b32 banks are (a / 4) mod 32 over 2 groups of 32 lanes.
    Returns LDS cycles per fragment (8 = conflict-free) over all rows of the tile and kernel rows."""
    worst = 0
    for w in range(4):
        for ky in range(5):
            for i in range(4):
                tot = 0
                for half in range(2):
                    for d in range(4):
                        banks = {}
                        for lane in range(32 * half, 32 * half + 32):
                            py, px, k = lane_pixel(lane)
                            a = ((4 * w + py + ky) * pitch + 4 * i + px) * pb + 16 * k + 4 * d
                            banks.setdefault((a // 4) % 32, set()).add(a)
                        tot += max(len(v) for v in banks.values())
                worst = max(worst, tot)
    return worst


def gemm_fragment_reads(pairs):
    """gemm.hip k_gemm<.., S16> fragment byte addresses per lane inside a ring group (4 slabs of 16 KB: A rows at
    row * 64, W rows at 8192 + row * 64, 16-B slot xor wsw(row) = 2 ((row >> 2) & 1)), for every wave (wm, wn), fragment
    and slab position: slab by slab (A slot kg; W slots kg & 1 and 2 + (kg & 1)) or the planar slab pairs (lanes of
    k-groups 2, 3 one slab further; h slots kg & 1, l slots 2 + (kg & 1) of A and of W).  Yields (name, [64 addresses])."""
    wsw = lambda row: 2 * ((row >> 2) & 1)
    for pos in (range(0, 4, 2) if pairs else range(4)):
        for wm in range(2):
            for i in range(4):
                rows = [64 * wm + 16 * i + (l & 15) for l in range(64)]
                if pairs:
                    for nm, s0 in (("A'h", 0), ("A'l", 2)):
                        yield f"{nm} pos {pos} wm {wm} i {i}", [
                            (pos + (l >> 5)) * 16384 + rows[l] * 64 + (((s0 + ((l >> 4) & 1)) ^ wsw(l & 15)) << 4) for l in range(64)]
                else:
                    yield f"A pos {pos} wm {wm} i {i}", [pos * 16384 + rows[l] * 64 + (((l >> 4) ^ wsw(l & 15)) << 4) for l in range(64)]
        for wn in range(4):
            for j in range(2):
                rows = [32 * wn + 16 * j + (l & 15) for l in range(64)]
                for nm, s0 in (("Wh", 0), ("Wl", 2)):
                    yield f"{nm} pos {pos} wn {wn} j {j}", [
                        (pos + ((l >> 5) if pairs else 0)) * 16384 + 8192 + rows[l] * 64 + (((s0 + ((l >> 4) & 1)) ^ wsw(l & 15)) << 4)
                        for l in range(64)]


def tail_fragment_reads(pairs):
    """conv_dects.hip k_dec_tail_s16 A fragment byte addresses per lane: 16 consecutive pixels q = 16 f + r16 of the
    10-wide grid at pixel pitch 18, d_deconv4 window pixels of 96 B (16 taps, 14 fragments), d_deconv5 image pixels of
    288 B (the phases' taps x 4 chunks of 64 B, 13 fragments); slab by slab a lane reads 16-B group kg, the planar pairs
    read group kg & 1 (h) or 2 + (kg & 1) (l) with k-groups 2, 3 on the next tap (one pixel lower: d_deconv4, every tap
    pair) or the next chunk (+ 64 B: d_deconv5, every chunk pair).  Yields (name, [64 addresses])."""
    def pix(f, l, pitch):
        q = 16 * f + (l & 15)
        return (q // 10) * 18 * pitch + (q % 10) * pitch
    for f in range(14):
        for t in (range(0, 16, 2) if pairs else range(16)):
            imm = ((3 - t // 4) * 18 + (3 - t % 4)) * 96
            if pairs:
                for nm, s0 in (("A'h", 0), ("A'l", 32)):
                    yield f"d4 {nm} f {f} taps {t},{t + 1}", [imm + s0 + pix(f, l, 96) + ((l >> 4) & 1) * 16 - (l >> 5) * 96 for l in range(64)]
            else:
                yield f"d4 A f {f} tap {t}", [imm + pix(f, l, 96) + (l >> 4) * 16 for l in range(64)]
    for f in range(13):
        for dy in range(3):
            for dx in range(3):
                for c in (range(0, 4, 2) if pairs else range(4)):
                    imm = (dy * 18 + dx) * 288 + c * 64
                    if pairs:
                        for nm, s0 in (("A'h", 0), ("A'l", 32)):
                            yield f"d5 {nm} f {f} tap ({dy},{dx}) chunks {c},{c + 1}", [
                                imm + s0 + pix(f, l, 288) + ((l >> 4) & 1) * 16 + (l >> 5) * 64 for l in range(64)]
                    else:
                        yield f"d5 A f {f} tap ({dy},{dx}) chunk {c}", [imm + pix(f, l, 288) + (l >> 4) * 16 for l in range(64)]
    # weight ring: 64 rows x 64 B per slab (4 KB), slot xor wsw(row); wave's rows 16 cb + r16
    wsw = lambda row: 2 * ((row >> 2) & 1)
    for cb in range(4):
        for pos in (range(0, 4, 2) if pairs else range(4)):
            for nm, s0 in (("Wh", 0), ("Wl", 2)):
                yield f"{nm} cb {cb} pos {pos}", [(pos + ((l >> 5) if pairs else 0)) * 4096 + (16 * cb + (l & 15)) * 64 +
                                                  (((s0 + ((l >> 4) & 1)) ^ wsw(16 * cb + (l & 15))) << 4) for l in range(64)]


def read_conflicts(addrs):
    """16-lane service groups of one ds_read_b128 that do not hit 16 distinct 16-B units of the 256-B bank line."""
    return sum(len({(addrs[l] // 16) % 16 for l in grp}) < 16 for grp in GROUPS)


if __name__ == "__main__":
    import sys
    if "--gemm" in sys.argv:
        for pairs in (False, True):
            reads = list(gemm_fragment_reads(pairs))
            assert all(0 <= a and a + 16 <= 65536 and a % 16 == 0 for _, ad in reads for a in ad), "inside the ring group"
            bad = [name for name, ad in reads if read_conflicts(ad)]
            assert not bad, bad[:8]
            print(f"k_gemm split fragments, {'planar slab pairs' if pairs else 'slab by slab'}: {len(reads)} reads "
                  f"(every wave, fragment and slab position), all conflict-free")
        sys.exit(0)
    if "--v1r" in sys.argv:
        for pitch in range(20, 29):
            print(f"conv_v1r window pitch {pitch}: {v1r_read2_cycles(pitch)} LDS cycles per A fragment (8 = conflict-free)")
        sys.exit(0)
    if "--tail" in sys.argv:
        for pairs in (False, True):
            reads = list(tail_fragment_reads(pairs))
            assert all(a >= 0 and a % 16 == 0 for _, ad in reads for a in ad)
            bad = [name for name, ad in reads if read_conflicts(ad)]
            assert not bad, bad[:8]
            print(f"k_dec_tail_s16 fragments, {'planar slab pairs' if pairs else 'slab by slab'}: {len(reads)} reads (every "
                  f"fragment, tap or tap pair, chunk or chunk pair, weight ring position), all conflict-free at pitch 18")
        sys.exit(0)
    assert all(max(g) < 32 or min(g) >= 32 for g in GROUPS), "a service group stays within one half of the wave"
    for name, kmap in KMAPS.items():
        assert halo_ok(lambda y: 2 * (y & 1), kmap), f"hsw<true>, {name}"
        assert weights_ok((0, 2, 0, 2), kmap), f"wswz<true>, {name}"
        print(f"{name}: halo and weight images conflict-free for every tap and all three geometries")
    assert not halo_ok(lambda y: y & 3)      # the 32x32x16 swizzle conflicts under the 16x16x32 layout
    print("halo swizzles (y mod 4 -> slot xor):", [t for t in itertools.product(range(4), repeat=4) if halo_ok(lambda y, t=t: t[y % 4])])
    print("weight swizzles ((co >> 2) mod 4 -> slot xor):", [t for t in itertools.product(range(4), repeat=4) if weights_ok(t)])
