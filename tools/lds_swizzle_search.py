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


if __name__ == "__main__":
    import sys
    if "--v1r" in sys.argv:
        for pitch in range(20, 29):
            print(f"conv_v1r window pitch {pitch}: {v1r_read2_cycles(pitch)} LDS cycles per A fragment (8 = conflict-free)")
        sys.exit(0)
    assert all(max(g) < 32 or min(g) >= 32 for g in GROUPS), "a service group stays within one half of the wave"
    for name, kmap in KMAPS.items():
        assert halo_ok(lambda y: 2 * (y & 1), kmap), f"hsw<true>, {name}"
        assert weights_ok((0, 2, 0, 2), kmap), f"wswz<true>, {name}"
        print(f"{name}: halo and weight images conflict-free for every tap and all three geometries")
    assert not halo_ok(lambda y: y & 3)      # the 32x32x16 swizzle conflicts under the 16x16x32 layout
    print("halo swizzles (y mod 4 -> slot xor):", [t for t in itertools.product(range(4), repeat=4) if halo_ok(lambda y, t=t: t[y % 4])])
    print("weight swizzles ((co >> 2) mod 4 -> slot xor):", [t for t in itertools.product(range(4), repeat=4) if weights_ok(t)])
