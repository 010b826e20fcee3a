"""CPU: libctseg_hip.so loads without a GPU and exports every symbol include/ctseg_hip.h declares; the ctypes
binding table covers exactly that set; argument validation rejects bad descriptors without touching a device."""
import ctypes
import os
import re

import pytest

from capstone_amd import _native as nat

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "ctseg_hip.h")


def _declared():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ctseg_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_are_exported_and_bound():
    names = _declared()
    assert len(names) >= 20
    lib = ctypes.CDLL(nat.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in ctseg_hip.h but not exported"
    assert sorted(nat.EXPORTS) == names


def test_host_side_queries_and_validation():
    L = nat.lib()
    hdr = int(re.search(r"#define CTSEG_ABI_VERSION (\d+)", open(HEADER).read()).group(1))
    assert L.ctseg_abi_version() == hdr == nat.ABI_VERSION == 3
    assert (L.ctseg_conv_tile_rows(10), L.ctseg_conv_tile_rows(256)) == (256, 128)
    assert [L.ctseg_conv_tile_cols(c) for c in (10, 32, 64, 256)] == [16, 32, 64, 128]
    assert [L.ctseg_wgrad_tile_cols(c) for c in (10, 32, 64, 256)] == [16, 32, 64, 128]
    d = nat.ConvDesc()                      # all-zero descriptor: rejected before any launch
    assert L.ctseg_conv_igemm(ctypes.byref(d), None) < 0
    assert b"null pointer" in L.ctseg_last_error()
    with pytest.raises(nat.NativeError):
        nat.check(-1, "x")


def test_descriptors_carry_their_struct_size_and_a_foreign_size_is_rejected():
    """ABI 2: both descriptor structs start with the sizeof() their caller was compiled against; a caller built against another
    header (round 2 appended fields under version 1) is refused by every entry point instead of being read past its end."""
    L = nat.lib()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for cname, cls in (("ctseg_conv_desc", nat.ConvDesc), ("ctseg_wgrad_desc", nat.WgradDesc)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), src, flags=re.S).group(1)
        first = [ln.strip() for ln in body.splitlines() if ln.strip()][0]
        assert first.startswith("int32_t struct_size"), first
        assert cls._fields_[0][0] == "struct_size" and cls().struct_size == ctypes.sizeof(cls)
        # every header field is mirrored, in order (names: `in` is spelled in_ in Python)
        names = re.findall(r"(?:\*|\s)([A-Za-z_][A-Za-z0-9_]*)(?:\[[A-Z_]+\])?\s*[,;]", body)
        assert [n if n != "in" else "in_" for n in names] == [f[0] for f in cls._fields_], (cname, names)
    d = nat.ConvDesc()
    d.struct_size -= 24                      # "compiled against the round-1 header"
    assert L.ctseg_conv_igemm(ctypes.byref(d), None) < 0 and b"struct_size" in L.ctseg_last_error()
    assert L.ctseg_conv_num_tiles(ctypes.byref(d)) < 0
    assert L.ctseg_conv_split_ok(ctypes.byref(d)) == 0 and L.ctseg_conv_narrow_ok(ctypes.byref(d)) == 0
    assert L.ctseg_conv_in_norm_ok(ctypes.byref(d)) == 0 and L.ctseg_conv_logits_ce_slots(ctypes.byref(d), 10) == 0
    w = nat.WgradDesc()
    w.struct_size += 8
    assert L.ctseg_conv_wgrad(ctypes.byref(w), None) < 0 and b"struct_size" in L.ctseg_last_error()
    assert L.ctseg_conv_wgrad_slabs(ctypes.byref(w)) < 0
    assert L.ctseg_wgrad_narrow_ok(ctypes.byref(w)) == 0 and L.ctseg_wgrad_in_norm_ok(ctypes.byref(w)) == 0


def test_product_has_no_cpu_fallback():
    import torch
    from capstone_amd.models import UNet
    net = UNet(3, 1, 10, (4, 8), (2,), num_res_units=2)
    with pytest.raises(nat.NativeError):
        net(torch.zeros(1, 1, 8, 8, 8))     # CPU tensor: loud failure, not an eager path
    with pytest.raises(nat.NativeError):
        net.model[0].conv.unit0(torch.zeros(1, 1, 8, 8, 8))   # containers never compute


def test_pack_block_structs_mirror_the_header():
    """ctseg_pack_block / ctseg_pack_part (ABI 3, ctseg_pack_weights): field order, array sizes and the struct size of the ctypes
    mirror follow the header (natural alignment on both sides)."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for cname, cls in (("ctseg_pack_part", nat.PackPart), ("ctseg_pack_block", nat.PackBlock)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), src, flags=re.S).group(1)
        names = re.findall(r"(?:\*|\s)([A-Za-z_][A-Za-z0-9_]*)(?:\[[A-Za-z_0-9]+\])?\s*[,;]", body)
        assert names == [f[0] for f in cls._fields_], (cname, names)
    assert ctypes.sizeof(nat.PackPart) == 32 and ctypes.sizeof(nat.PackBlock) == 8 + 4 * 4 + 8 + 2 * 32 + 4 * nat.MAX_TAPS + 4
    assert int(re.search(r"#define CTSEG_PACK_LDS_FLOATS (\d+)", open(HEADER).read()).group(1)) == nat.PACK_LDS_FLOATS


def test_weight_gradient_sizing_query_and_the_split_model():
    """ctseg_conv_wgrad_wgs_per_slab (host-side, no GPU): which kernel a descriptor gets and what one slab of it costs; and the split
    count capstone_amd.engine.GemmLayer._wgrad_splits derives from it for the many-channel layers of the reference's network
    (UNet(3,1,10,(32,64,128,256),(2,2,2,2),2) on 2x1x512x512x48, /root/reference/capstone/volumetric/base_trainer.py:65-72)."""
    import types
    from capstone_amd.engine import GemmLayer
    L = nat.lib()

    def desc(cg, cn, rows, sin=1, dt=nat.BF16, taps=27, N=2):
        d = nat.WgradDesc()
        d.dtype = dt
        d.in_, d.dy = 4096, 8192                       # (only their alignment is looked at)
        d.N = N
        d.Xr, d.Yr, d.Zr = rows
        d.Xi, d.Yi, d.Zi = [r * sin for r in rows]
        d.Cg, d.Cn, d.g_ld, d.d_ld, d.sin, d.ntaps = cg, cn, cg, cn, sin, taps
        bnw = L.ctseg_wgrad_tile_cols(cn)
        d.splits, d.kpad_w, d.cn_pad = 1, -(-(taps * cg + 1) // 128) * 128, -(-cn // bnw) * bnw
        return d

    def ask(d):
        pc, sb = ctypes.c_int32(-1), ctypes.c_int32(-1)
        return L.ctseg_conv_wgrad_wgs_per_slab(ctypes.byref(d), ctypes.byref(pc), ctypes.byref(sb)), pc.value, sb.value

    # ring kernel: 256 x 256 tile (cn_pad % 256 == 0), 256 x 128, 512 x 64; one workgroup per CU; bytes of a 32-row stage
    assert ask(desc(256, 256, (64, 64, 6))) == (28, 1, 32 * 512 * 2)          # 27 K tiles + the bias row's own
    assert ask(desc(128, 128, (64, 64, 6))) == (14, 1, 32 * 384 * 2)
    assert ask(desc(64, 384, (64, 64, 6), sin=2)) == (7 * 3, 1, 32 * 384 * 2)
    assert ask(desc(64, 64, (128, 128, 12))) == (4, 1, 32 * 576 * 2)
    # fp32 storage and the few-channel layers keep the generic kernel (four 128-row tiles per CU) ...
    assert ask(desc(64, 64, (128, 128, 12), dt=nat.F32)) == (14, 4, 32 * (128 + 64) * 4)
    assert ask(desc(48, 40, (40, 40, 20)))[1] == 4
    # ... persistent LDS-halo kernels size their own grid
    assert ask(desc(32, 32, (256, 256, 24))) == (0, 0, 0)
    z = nat.WgradDesc()
    z.struct_size = 8
    assert L.ctseg_conv_wgrad_wgs_per_slab(ctypes.byref(z), None, None) < 0

    stub = types.SimpleNamespace(plan=types.SimpleNamespace(dt=nat.BF16))
    for cg, cn, rows, sin in ((256, 256, (64, 64, 6), 1), (128, 256, (64, 64, 6), 1), (64, 64, (128, 128, 12), 1), (32, 128, (128, 128, 12), 2)):
        d = desc(cg, cn, rows, sin)
        s = GemmLayer._wgrad_splits(stub, d, 2, rows[0] * rows[1] * rows[2], False)
        wps = ask(d)[0]
        assert 1 <= s and rows[0] * rows[1] * rows[2] // s >= 192, (cg, cn, s)
        assert 192 <= wps * 2 * s <= 256, (cg, cn, s, wps * 2 * s)           # one nearly full round of 256 workgroups
    # the generic rule is untouched (fp32 storage: 2048 workgroups aimed for, slabs in multiples of 8)
    stub32 = types.SimpleNamespace(plan=types.SimpleNamespace(dt=nat.F32))
    assert GemmLayer._wgrad_splits(stub32, desc(64, 64, (128, 128, 12), dt=nat.F32), 2, 128 * 128 * 12, False) == 72


def _conv_desc(dt, cg, cn, rows, kind="plain", g_ld=None):
    """a hand-filled forward descriptor (no memory behind the pointers: the host queries look at their alignment only).
    kind: "plain" 3x3x3 stride 1, "down" 3x3x3 stride 2, "up" the 8 parity classes of a stride-2 transposed convolution"""
    from capstone_amd.engine import classes_plain, classes_up
    e, bk = nat.epc(dt), 128 // nat.elsize(dt)
    d = nat.ConvDesc()
    d.in_, d.w, d.out, d.dtype = 4096, 1 << 20, 1 << 24, dt
    d.N = 2
    d.Xr, d.Yr, d.Zr = rows
    sin, sout = (2, 1) if kind == "down" else (1, 2) if kind == "up" else (1, 1)
    d.Xi, d.Yi, d.Zi = [r * sin for r in rows]
    d.Xo, d.Yo, d.Zo = [r * sout for r in rows]
    d.sin, d.sout = sin, sout
    d.Cg, d.Cn, d.Cn_store = cg, cn, -(-cn // e) * e
    d.g_ld, d.o_ld = g_ld or cg, d.Cn_store
    classes = classes_up(3, 3) if kind == "up" else classes_plain(3, 3, lambda t: t - 1)
    d.nclass = len(classes)
    rows_pad, off = -(-cn // 128) * 128, 0
    for i, ((ox, oy, oz), taps) in enumerate(classes):
        c = d.cls[i]
        c.ntaps, c.kpad, c.w_off = len(taps), -(-len(taps) * cg // bk) * bk, off
        c.ox, c.oy, c.oz = ox, oy, oz
        for j, (_, o) in enumerate(taps):
            c.taps[j] = o
        off += rows_pad * c.kpad
    return d


PASS_NAME_CASES = [
    # one descriptor per kernel family, in the order the library tries them ...
    ("x-column halo", nat.BF16, 16, 16, (9, 11, 13), "plain", None),
    ("halo", nat.F32, 16, 16, (9, 11, 13), "plain", None),
    ("up", nat.BF16, 64, 10, (7, 9, 5), "up", None),
    ("stem", nat.BF16, 1, 32, (5, 6, 10), "down", None),
    ("streamed-weight halo", nat.BF16, 64, 64, (9, 20, 13), "plain", None),
    ("streamed-weight halo", nat.BF16, 128, 32, (9, 20, 12), "up", None),
    ("stride-2 halo", nat.BF16, 16, 64, (18, 10, 12), "down", None),
    ("stride-2 register-weight", nat.BF16, 32, 128, (9, 20, 12), "down", None),
    ("many-channel 8-class", nat.BF16, 256, 64, (9, 20, 12), "up", None),
    # ... and one per tile of the generic family
    ("generic 256x16", nat.BF16, 40, 12, (7, 9, 11), "plain", None),
    ("generic 256x32", nat.BF16, 40, 24, (7, 9, 11), "plain", None),
    ("generic 128x64", nat.BF16, 40, 48, (7, 9, 11), "plain", None),
    ("generic 128x128", nat.BF16, 40, 96, (7, 9, 11), "plain", None),
    ("generic 192x256", nat.BF16, 40, 160, (7, 9, 11), "plain", None),
    ("generic ring 192x128", nat.BF16, 128, 128, (7, 9, 11), "plain", None),
    ("generic ring 192x256", nat.BF16, 256, 256, (5, 6, 7), "plain", None),
    # what moves a shape off its family: storage, size, row layout
    ("generic 256x32", nat.F32, 32, 32, (5, 9, 13), "plain", None),             # fp32 voxels of 128 bytes: not the halo kernel
    ("generic 128x64", nat.BF16, 256, 64, (5, 9, 6), "up", None),               # < 2048 rows: not the many-channel 8-class kernel
    ("generic 256x32", nat.BF16, 128, 32, (6, 10, 7), "up", None),              # < 2048 rows: not the streamed-weight halo kernel
    ("x-column halo", nat.BF16, 16, 10, (7, 11, 13), "plain", 12),              # 12-wide gathered rows
    ("generic 128x64", nat.F32, 24, 48, (7, 9, 11), "plain", None),
]


@pytest.mark.parametrize("name,dt,cg,cn,rows,kind,g_ld", PASS_NAME_CASES, ids=[f"{c[0]} {c[2]}->{c[3]} {c[5]}" + (" fp32" if c[1] == nat.F32 else "") for c in PASS_NAME_CASES])
def test_conv_pass_name_per_family_and_generic_tile(name, dt, cg, cn, rows, kind, g_ld):
    L = nat.lib()
    d = _conv_desc(dt, cg, cn, rows, kind, g_ld)
    got = L.ctseg_conv_pass_name(ctypes.byref(d))
    assert got is not None and got.decode() == name


def test_conv_pass_name_follows_the_extras_and_rejects_bad_descriptors(monkeypatch):
    L = nat.lib()
    d = _conv_desc(nat.BF16, 32, 128, (9, 20, 12), "down")
    assert L.ctseg_conv_pass_name(ctypes.byref(d)) == b"stride-2 register-weight"
    d.add, d.add_ld = 1 << 26, 128               # that kernel takes no addend: the launch (and the name) move on
    assert L.ctseg_conv_pass_name(ctypes.byref(d)) == b"generic 128x128"
    d.add = None
    monkeypatch.setenv("CTSEG_NO_DOWN_R", "1")   # the selector's own switch is honoured: the name is what WOULD run
    assert L.ctseg_conv_pass_name(ctypes.byref(d)) == b"generic 128x128"
    monkeypatch.delenv("CTSEG_NO_DOWN_R")
    x = _conv_desc(nat.BF16, 16, 10, (7, 11, 13), "plain")
    x.out_f32, x.Cn_store, x.o_ld = 1, 12, 12
    assert L.ctseg_conv_pass_name(ctypes.byref(x)) == b"x-column halo"
    assert L.ctseg_conv_pass_name(ctypes.byref(nat.ConvDesc())) is None          # empty dims
    assert L.ctseg_conv_pass_name(None) is None
    bad = _conv_desc(nat.BF16, 16, 16, (9, 11, 13))
    bad.struct_size -= 8
    assert L.ctseg_conv_pass_name(ctypes.byref(bad)) is None
    bad = _conv_desc(nat.BF16, 16, 16, (9, 11, 13))
    bad.nclass = 9
    assert L.ctseg_conv_pass_name(ctypes.byref(bad)) is None
    bad = _conv_desc(nat.BF16, 16, 16, (9, 11, 13))
    bad.dtype = nat.U8
    assert L.ctseg_conv_pass_name(ctypes.byref(bad)) is None


def _ceil_to(v, m):
    return -(-v // m) * m


def _tile_axis_rule(rows, ta, orders):
    """The kernels' choice of tile axes, restated: a tile is ta x 8 x 8 along (a, b, c); the first order stands unless a later one
    pads the row grid to a strictly smaller volume (by more than 1e-9 of the grid).  -> (order, tiles per sample of every order)"""
    full = float(rows[0]) * rows[1] * rows[2]
    waste = [float(_ceil_to(rows[a], ta)) * _ceil_to(rows[b], 8) * _ceil_to(rows[c], 8) / full for a, b, c in orders]
    tiles = [(_ceil_to(rows[a], ta) // ta) * (_ceil_to(rows[b], 8) // 8) * (_ceil_to(rows[c], 8) // 8) for a, b, c in orders]
    pick, best = 0, waste[0]
    for i in range(1, len(orders)):
        if waste[i] < best - 1e-9:
            pick, best = i, waste[i]
    return orders[pick], tiles


XYZ, ZXY, YXZ = (0, 1, 2), (2, 0, 1), (1, 0, 2)
# (family, Cg, Cn, kind, tile depth along a, candidate orders in the kernels' preference, tiles reported per tile of the grid)
TILE_FAMILIES = {
    "sw64": ("streamed-weight halo", 64, 64, "plain", 4, (XYZ, ZXY), 1),
    "sw8": ("streamed-weight halo", 128, 32, "up", 4, (XYZ, ZXY), 1),
    "down": ("stride-2 halo", 16, 64, "down", 4, (XYZ, ZXY), 1),
    "up8": ("many-channel 8-class", 256, 64, "up", 3, (XYZ, ZXY), 2),       # two class groups: twice its per-group grid
    "down_r": ("stride-2 register-weight", 32, 128, "down", 1, (XYZ, ZXY, YXZ), 1),
}
# (family, row grid, the order the rule picks (derived by hand), tiles of that order, tiles of the first order)
TILE_AXIS_CASES = [
    ("sw64", (229, 3, 3), ZXY, 29, 58),
    ("sw64", (9, 20, 13), XYZ, 18, 18),
    ("sw8", (16, 16, 12), ZXY, 12, 16),
    ("sw8", (9, 20, 12), XYZ, 18, 18),         # an exact tie: both orders pad to 4608 voxels; the first one stays
    ("down", (18, 10, 12), ZXY, 18, 20),
    ("up8", (16, 16, 9), ZXY, 12, 24),
    ("up8", (9, 20, 12), XYZ, 18, 18),
    ("down_r", (8, 16, 17), ZXY, 17 * 2, 8 * 2 * 3),      # z is the 1-deep axis: the (x, y) face needs no padding
    ("down_r", (8, 17, 16), YXZ, 17 * 2, 8 * 3 * 2),      # y is
    ("down_r", (9, 20, 12), XYZ, 9 * 3 * 2, 9 * 3 * 2),   # x is: (y, z) pads 20 x 12 to 24 x 16 = 1.6, (x, y) 2.13, (x, z) 2.37
]


@pytest.mark.parametrize("fam,rows,order,tiles,tiles_first", TILE_AXIS_CASES, ids=[f"{c[0]} {c[1]}" for c in TILE_AXIS_CASES])
def test_tile_axis_choice_matches_the_padding_rule(fam, rows, order, tiles, tiles_first, monkeypatch):
    monkeypatch.delenv("CTSEG_MAX_WG", raising=False)
    name, cg, cn, kind, ta, orders, per_tile = TILE_FAMILIES[fam]
    want_order, all_tiles = _tile_axis_rule(rows, ta, orders)
    # the table's hand-derived figures against the restated rule, then the rule against the library
    assert want_order == order and all_tiles[orders.index(order)] == tiles and all_tiles[0] == tiles_first
    if order != XYZ:
        assert all(t != tiles for o, t in zip(orders, all_tiles) if o != order)      # a wrong choice shows in the count
    L = nat.lib()
    d = _conv_desc(nat.BF16, cg, cn, rows, kind)
    d.N = 1
    assert L.ctseg_conv_pass_name(ctypes.byref(d)) == name.encode()
    assert L.ctseg_conv_num_tiles(ctypes.byref(d)) == per_tile * tiles


def test_tile_axis_tie_stays_xyz():
    """8-class rows (9, 20, 12) at a tile depth of 4 pad to 12 x 24 x 16 = 12 x 16 x 24 = 4608 voxels in either order: an exact tie"""
    assert _ceil_to(9, 4) * _ceil_to(20, 8) * _ceil_to(12, 8) == _ceil_to(12, 4) * _ceil_to(9, 8) * _ceil_to(20, 8) == 4608
    assert _tile_axis_rule((9, 20, 12), 4, (XYZ, ZXY))[0] == XYZ


def _wgrad_desc(dt, cg, cn, rows, sin=1, g_ld=None, d_ld=None, k=3, dims=3, N=2):
    """a hand-filled weight-gradient descriptor (no memory behind the pointers: null `in` / `dy` are 16-byte aligned).  For a
    transposed convolution the caller passes the gathered side (dOut: cg = its channel stride) and cn = the layer's input channels"""
    from capstone_amd.engine import classes_plain
    L = nat.lib()
    d = nat.WgradDesc()
    d.dtype, d.N = dt, N
    d.Xr, d.Yr, d.Zr = rows
    d.Xi, d.Yi, d.Zi = [r * sin if i < dims else 1 for i, r in enumerate(rows)]
    d.Cg, d.Cn, d.g_ld, d.d_ld, d.sin = cg, cn, g_ld or cg, d_ld or -(-cn // nat.epc(dt)) * nat.epc(dt), sin
    taps = classes_plain(k, dims, lambda t: t - (k - 1) // 2)[0][1]
    d.ntaps = len(taps)
    for j, (_, off) in enumerate(taps):
        d.taps[j] = off
    bnw = L.ctseg_wgrad_tile_cols(cn)
    d.splits, d.kpad_w, d.cn_pad = 1, -(-(d.ntaps * cg + 1) // 128) * 128, -(-cn // bnw) * bnw
    return d


def _wgrad_name(d):
    got = nat.lib().ctseg_wgrad_pass_name(ctypes.byref(d))
    return None if got is None else got.decode()


B, F = nat.BF16, nat.F32
WGRAD_NAME_CASES = [
    # (name, dtype, Cg, Cn, rows, keyword arguments of _wgrad_desc)
    ("x-column head 12/12", B, 16, 10, (5, 9, 13), dict(g_ld=12, d_ld=12)),
    ("x-column head 12/16", B, 16, 10, (5, 9, 13), dict(g_ld=12, d_ld=16)),
    ("x-column head 16/12", B, 16, 10, (5, 9, 13), dict(g_ld=16, d_ld=12)),
    ("x-column head 16/16", B, 16, 16, (5, 9, 13), {}),
    ("x-column head 16/16", B, 16, 16, (5, 9, 4), {}),                       # Z = 4: the eligibility edge
    ("generic 16", B, 16, 16, (5, 9, 3), {}),                                # Z = 3: below it
    ("halo 32x32", B, 16, 16, (5, 9, 13), dict(g_ld=24)),                    # rows neither 12 nor 16 wide
    ("halo 32x64", B, 16, 32, (5, 9, 13), {}),
    ("halo 64x32", B, 32, 16, (5, 9, 13), {}),
    ("halo 64x32", B, 32, 10, (5, 9, 13), {}),
    ("halo 64x64", B, 32, 32, (5, 9, 13), {}),
    ("halo 64x64", B, 32, 24, (4, 8, 8), dict(d_ld=32)),                     # pad columns inside a 16-column block ...
    ("generic 32", B, 32, 24, (4, 8, 8), {}),                                # ... but dY rows of 24 are narrower than its planes
    ("up 16", B, 16, 64, (5, 6, 9), dict(sin=2)),
    ("up 12", B, 16, 64, (1, 2, 3), dict(sin=2, g_ld=12)),
    ("stem 16", B, 1, 16, (4, 6, 4), dict(sin=2)),
    ("stem 32", B, 1, 32, (4, 6, 4), dict(sin=2)),
    ("stem 48", B, 1, 48, (5, 10, 12), dict(sin=2)),
    ("stem 64", B, 1, 64, (5, 10, 12), dict(sin=2)),
    ("ring 256x256", B, 64, 256, (6, 6, 6), {}),
    ("ring 256x128", B, 32, 128, (6, 8, 4), dict(sin=2)),
    ("ring 512x64", B, 64, 64, (7, 10, 6), {}),
    ("generic 16", B, 8, 8, (5, 9, 13), {}),
    ("generic 32", B, 24, 24, (5, 9, 13), {}),
    ("generic 64", B, 48, 48, (5, 9, 13), {}),
    ("generic 64", B, 96, 40, (5, 9, 13), {}),
    ("generic 128", B, 24, 160, (5, 9, 13), {}),                             # (96 -> 160 in bf16 is the ring's)
    ("ring 256x256", B, 96, 160, (5, 9, 13), {}),
    ("generic 16", F, 8, 8, (5, 9, 13), {}),
    ("generic 32", F, 24, 24, (5, 9, 13), {}),
    ("generic 64", F, 48, 48, (5, 9, 13), {}),
    ("generic 64", F, 96, 40, (5, 9, 13), {}),
    ("generic 128", F, 96, 160, (5, 9, 13), {}),
    ("generic 32", F, 16, 32, (5, 9, 13), {}),                               # fp32 storage: never an LDS-halo kernel
    ("generic 32", B, 48, 24, (5, 9, 13), dict(k=1)),                        # 1x1x1
    ("generic 32", B, 16, 32, (8, 8, 1), dict(sin=2, k=3, dims=2)),          # Conv2d 16 -> 32 s2
    ("generic 32", B, 16, 32, (4, 4, 1), dict(sin=2, k=3, dims=2)),          # ConvTranspose2d 32 -> 16 s2: gathers dOut, 32 columns
    ("generic 16 element-wise", B, 3, 16, (9, 13, 1), dict(dims=2)),         # Conv2d 3 -> 16: gathered rows of 6 bytes
    ("generic 16 element-wise", F, 1, 16, (4, 6, 4), dict(sin=2)),           # fp32 first layer: not the (bf16) stem kernel
    ("generic 16 element-wise", F, 6, 8, (5, 9, 13), {}),
    ("generic 32 element-wise", B, 3, 32, (9, 13, 1), dict(dims=2)),
    ("generic 64 element-wise", B, 3, 40, (9, 13, 1), dict(dims=2)),
    ("generic 128 element-wise", F, 6, 96, (5, 9, 13), {}),
]


@pytest.mark.parametrize("name,dt,cg,cn,rows,kw", WGRAD_NAME_CASES,
                         ids=[f"{c[0]} {c[2]}->{c[3]} {c[4]}" + (" fp32" if c[1] == nat.F32 else "") for c in WGRAD_NAME_CASES])
def test_wgrad_pass_name_per_instantiation(name, dt, cg, cn, rows, kw):
    assert _wgrad_name(_wgrad_desc(dt, cg, cn, rows, **kw)) == name


def test_wgrad_pass_name_of_the_non_canonical_head_and_the_on_load_variants():
    """conv_wgrad_head_kernel (the head kernel without the x-column reuse) serves only taps out of canonical order, which no layer of
    the host mirror records: reachable by a hand-made descriptor alone.  The dyn variants of the stem kernel follow dyn_g."""
    for gw in (12, 16):
        for dw in (12, 16):
            d = _wgrad_desc(B, 16, 10, (5, 9, 13), g_ld=gw, d_ld=dw)
            d.taps[0], d.taps[26] = d.taps[26], d.taps[0]
            assert _wgrad_name(d) == f"head {gw}/{dw}"
            assert nat.lib().ctseg_wgrad_in_norm_ok(ctypes.byref(d)) == 0
    for cn in (32, 64):
        d = _wgrad_desc(B, 1, cn, (4, 6, 4), sin=2, d_ld=cn // 2)
        d.dyn_col0, d.dyn_g, d.dyn_y, d.dyn_g_ld, d.dyn_y_ld = cn // 2, 1 << 20, 1 << 21, cn // 2, cn // 2
        d.dyn_mean_rstd = d.dyn_alpha = d.dyn_sums = 1 << 22
        assert nat.lib().ctseg_wgrad_dy_norm_ok(ctypes.byref(d)) == 1
        assert _wgrad_name(d) == f"stem {cn} dyn"
        d.N = 9                                     # the launch refuses it: no name
        assert _wgrad_name(d) is None
    d = _wgrad_desc(B, 1, 48, (4, 6, 4), sin=2, d_ld=24)
    d.dyn_col0, d.dyn_g, d.dyn_y, d.dyn_g_ld, d.dyn_y_ld = 24, 1 << 20, 1 << 21, 24, 24
    assert _wgrad_name(d) is None
    d = _wgrad_desc(B, 1, 32, (4, 6, 4), sin=2)
    d.dyn_col0 = 16                                 # dyn_col0 without dyn_g
    assert _wgrad_name(d) is None
    # in_mean_rstd: the x-column head kernel only
    d = _wgrad_desc(B, 16, 10, (5, 9, 13), g_ld=12, d_ld=12)
    d.in_mean_rstd, d.in_alpha, d.in_norm_C = 1 << 20, 1 << 21, 10
    assert _wgrad_name(d) == "x-column head 12/12"
    d = _wgrad_desc(B, 32, 32, (5, 9, 13))
    d.in_mean_rstd, d.in_alpha, d.in_norm_C = 1 << 20, 1 << 21, 10
    assert _wgrad_name(d) is None
    # what the launch refuses beyond the queries has no name either (the two share wgrad_refusal)
    d = _wgrad_desc(B, 16, 10, (5, 9, 13), g_ld=12, d_ld=12)
    d.in_mean_rstd, d.in_norm_C = 1 << 20, 10       # no in_alpha
    assert _wgrad_name(d) is None
    d = _wgrad_desc(B, 1, 32, (4, 6, 4), sin=2, d_ld=16)
    d.dyn_col0, d.dyn_g, d.dyn_y, d.dyn_g_ld, d.dyn_y_ld = 16, 1 << 20, 1 << 21, 16, 16      # no table pointers
    assert _wgrad_name(d) is None
    d.dyn_mean_rstd = d.dyn_alpha = d.dyn_sums = 1 << 22
    d.dyn_g = (1 << 20) + 8                         # dyn_g not 16-byte aligned
    assert _wgrad_name(d) is None
    d = _wgrad_desc(B, 48, 48, (5, 9, 13), d_ld=52)  # dY rows not 16-byte chunked
    assert _wgrad_name(d) is None
    d = _wgrad_desc(B, 48, 48, (5, 9, 13))
    d.splits = 0
    assert _wgrad_name(d) is None


def test_wgrad_pass_name_honours_the_switches_and_rejects_bad_descriptors(monkeypatch):
    L = nat.lib()
    up = _wgrad_desc(B, 16, 64, (5, 6, 9), sin=2)
    up12 = _wgrad_desc(B, 16, 64, (5, 6, 9), sin=2, g_ld=12)
    ring = _wgrad_desc(B, 64, 256, (6, 6, 6))
    assert (_wgrad_name(up), _wgrad_name(up12), _wgrad_name(ring)) == ("up 16", "up 12", "ring 256x256")
    monkeypatch.setenv("CTSEG_NO_WGRAD_UP", "1")
    assert _wgrad_name(up) == "generic 64"
    assert _wgrad_name(up12) is None                # 12-wide rows on the generic kernel: the launch refuses
    assert L.ctseg_wgrad_narrow_ok(ctypes.byref(up12)) == 0
    monkeypatch.delenv("CTSEG_NO_WGRAD_UP")
    monkeypatch.setenv("CTSEG_WGRAD_RING", "0")
    assert _wgrad_name(ring) == "generic 128"
    assert _wgrad_name(_wgrad_desc(B, 64, 64, (7, 10, 6))) == "generic 64"
    monkeypatch.setenv("CTSEG_WGRAD_RING", "1")
    assert _wgrad_name(ring) == "ring 256x256"
    monkeypatch.delenv("CTSEG_WGRAD_RING")
    assert _wgrad_name(nat.WgradDesc()) is None                                # empty dims
    assert L.ctseg_wgrad_pass_name(None) is None
    bad = _wgrad_desc(B, 16, 16, (5, 9, 13))
    bad.struct_size -= 8
    assert _wgrad_name(bad) is None
    bad = _wgrad_desc(B, 16, 16, (5, 9, 13))
    bad.dtype = nat.F16                                                        # no weight-gradient kernels for IEEE half
    assert _wgrad_name(bad) is None
    bad = _wgrad_desc(B, 16, 16, (5, 9, 13))
    bad.ntaps = 28
    assert _wgrad_name(bad) is None


def test_wgrad_reduce_batch_ok_conditions():
    L = nat.lib()
    ok = L.ctseg_conv_wgrad_reduce_batch_ok
    assert ok(4096, 16, 0, 10) == 1 and ok(4096, 32, 16, 14) == 1
    assert ok(4096, 16, 2, 10) == 0                 # col0 % 4
    assert ok(4096, 18, 0, 10) == 0                 # cn_pad % 4
    assert ok(4100, 16, 0, 10) == 0                 # ws at a 4-byte offset
    assert ok(4096, 16, 8, 10) == 0                 # col0 + roundup(nb, 4) > cn_pad


def test_default_2d_unet_conv_passes_by_name():
    """every conv pass the default BaseUNet2D (filters 64 .. 1024, residual units, bf16) records, with the kernel the selector names
    for it, against the committed table (tests/unet2d_passes.py): a selector or recorder change shows as a named diff, row by row.
    At Z = 1 only the generic tiles and the ring kernel may appear: every other family needs 4 rows along z, 27 taps or 8 classes."""
    from unet2d_passes import UNET2D_PASSES, recorded_passes
    got = recorded_passes()
    diff = [(i, g, w) for i, (g, w) in enumerate(zip(got, UNET2D_PASSES)) if g != w]
    assert not diff, "\n".join(f"row {i}: recorded {g}\n        table    {w}" for i, g, w in diff)
    assert len(got) == len(UNET2D_PASSES) == 56, (len(got), len(UNET2D_PASSES))
    for pas, layer, *_, name in got:
        assert name is not None, (pas, layer, "the selector names no kernel")
        assert name.startswith("generic ") if pas != "wgrad" else name.startswith(("generic ", "ring ")), (pas, layer, name)
