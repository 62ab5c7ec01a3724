"""CPU: what the 3x3 / 3x3x3 convolution entry points accept and reject, and with which message (csrc/conv3x3_host.h and the
form-specific checks of conv3x3.hip, conv3x3_bf16.hip, conv3x3_f16.hip).

All of it runs before the first HIP call, so it is checked without a device and with pointers that are never dereferenced: a rejected
call returns -1 with its message; a call that passes validation fails at `hipGetDevice`, and its message then names that call.
Every row changes one thing of an accepted base case.  The return codes and message heads are those of the commit before the three
launchers were merged, with one deliberate difference: a tile count that wrapped in 32-bit arithmetic (H = W = 2^20) was accepted
and is rejected now ("too many tiles")."""
import pytest

from stardist_amd.lib import _native as N

P = 0x10000                       # "pointers": 16-byte aligned, distinct, never dereferenced
SRC0, SRC1, WP, BIAS, RES, OUT, FLAG, DOTW, DOTP = (P * k for k in range(1, 10))

BASE = dict(src0=SRC0, c0=32, stride0=32, up0=0, src1=None, c1=0, stride1=0, up1=0, D=1, H=8, W=8, kz=1, wp=WP, bias=BIAS,
            res=None, res_stride=0, c_out=32, act=1, out=OUT, flag=None, in_split=0, out_split=0, dotw=None, dotp=None)

# entry point -> (message prefix, argument order)
_COMMON = "src0 c0 stride0 up0 src1 c1 stride1 up1 D H W kz wp bias"
ENTRY = {
    "sd_conv3_res_ndhwc_device": ("sd_conv3_ndhwc", _COMMON + " res res_stride c_out act out"),
    "sd_conv3_bf16x6_res_ndhwc_device": ("sd_conv3_bf16x6", _COMMON + " res res_stride c_out act out"),
    "sd_conv3_f16x3_res_ndhwc_device": ("sd_conv3_f16x3", _COMMON + " res res_stride c_out act out flag"),
    "sd_conv3_f16x3_dot_ndhwc_device": ("sd_conv3_f16x3", _COMMON + " c_out act out flag dotw dotp"),
    "sd_conv3_f16x3_fmt_ndhwc_device": ("sd_conv3_f16x3", "src0 c0 up0 src1 c1 up1 D H W kz wp bias c_out act out in_split out_split flag dotw dotp"),
}
RES3 = ("sd_conv3_res_ndhwc_device", "sd_conv3_bf16x6_res_ndhwc_device", "sd_conv3_f16x3_res_ndhwc_device")
F16 = "sd_conv3_f16x3_res_ndhwc_device"
FMT = "sd_conv3_f16x3_fmt_ndhwc_device"
DOT = "sd_conv3_f16x3_dot_ndhwc_device"

ARGS = "unsupported channel counts (%d + %d -> %d), kz, act or misaligned pointers"
UP = "up is a bit mask"
SOURCES = "sources must hold multiples of 32 channels"
RESIDUAL = "the residual needs"
TILES = "too many tiles"
ROW = "an image row of"                      # "... %d pixels is too long for 32-bit offsets"
SPLIT = "split16 tensors are dense"
HEAD = "the fused head needs both"
ACCEPTED = "hipGetDevice"                    # passed every check: the first HIP call fails without a device
TWO = dict(src1=SRC1, c1=32, stride1=32)     # a second source


@pytest.fixture(scope="module")
def lib():
    l = N.lib()
    if l.sd_device_count() > 0:
        pytest.skip("a GPU is present: an accepted call would launch a kernel on these pointers")
    return l


def call(lib, entry, **changes):
    a = dict(BASE, **changes)
    if entry == FMT:                         # split16 tensors are dense: this entry point takes no strides
        assert a["stride0"] == a["c0"] and (a["src1"] is None or a["stride1"] == a["c1"]) and a["res"] is None
    elif entry == DOT:
        assert a["res"] is None and not a["in_split"] and not a["out_split"]
    else:
        assert a["dotw"] is None and a["dotp"] is None and not a["in_split"] and not a["out_split"]
    if not entry.startswith("sd_conv3_f16x3"):
        assert a["flag"] is None
    rc = getattr(lib, entry)(*[a[k] for k in ENTRY[entry][1].split()], None)
    return rc, lib.sd_last_error().decode(), a


def expect(lib, entry, want, **changes):
    rc, msg, a = call(lib, entry, **changes)
    prefix = ENTRY[entry][0]
    if want is None:
        assert rc == 0, (entry, changes, msg)
    elif want == ACCEPTED:
        assert rc == -1 and ACCEPTED in msg and not msg.startswith("sd_conv3"), (entry, changes, msg)
    else:
        if want == ARGS:
            want = ARGS % (a["c0"], a["c1"] if a["src1"] else 0, a["c_out"])
        assert rc == -1 and msg.startswith(prefix + ": " + want), (entry, changes, msg)


# (what changes, expected message head; None: nothing to do, rc 0)
SHARED_ROWS = [
    (dict(W=0), None),
    (dict(H=0), None),
    (dict(D=0), None),
    (dict(), ACCEPTED),
    (dict(bias=None), ACCEPTED),
    (dict(act=0), ACCEPTED),
    (dict(D=4, kz=3), ACCEPTED),
    (dict(H=9, W=33, c_out=64), ACCEPTED),
    (dict(TWO, up0=7, D=2, kz=3), ACCEPTED),
    (dict(stride0=36), ACCEPTED),
    (dict(res=RES, res_stride=32), ACCEPTED),
    (dict(src0=None), ARGS),
    (dict(wp=None), ARGS),
    (dict(out=None), ARGS),
    (dict(out=OUT + 4), ARGS),
    (dict(src0=SRC0 + 8), ARGS),
    (dict(bias=BIAS + 4), ARGS),
    (dict(TWO, src1=SRC1 + 4), ARGS),
    (dict(act=2), ARGS),
    (dict(kz=2), ARGS),
    (dict(kz=1, D=2), ARGS),
    (dict(c0=48, stride0=48), ARGS),
    (dict(c0=544, stride0=544), ARGS),
    (dict(c_out=48), ARGS),
    (dict(c_out=0), ARGS),
    (dict(TWO, c1=48, stride1=48), ARGS),
    (dict(TWO, c0=512, stride0=512), ARGS),
    (dict(up0=8), UP),
    (dict(up0=-1), UP),
    (dict(up0=1, W=7), UP),
    (dict(up0=2, H=7), UP),
    (dict(up0=4, D=3, kz=3), UP),
    (dict(TWO, up1=1, W=7), UP),
    (dict(stride0=28), SOURCES),
    (dict(stride0=34), SOURCES),
    (dict(TWO, stride1=16), SOURCES),
    (dict(res=RES, res_stride=16), RESIDUAL),
    (dict(res=RES, res_stride=34), RESIDUAL),
    (dict(res=RES + 4, res_stride=32), RESIDUAL),
    # the first failing check decides the message
    (dict(act=2, up0=8, stride0=28), ARGS),
    (dict(up0=8, stride0=28), UP),
    (dict(D=64, H=131072, W=131072, kz=3), TILES),       # 2^32 tiles
    (dict(H=1 << 20, W=1 << 20), TILES),                 # 2^32 tiles in one plane: the count wrapped to 0 in 32-bit arithmetic
]


@pytest.mark.parametrize("entry", RES3)
@pytest.mark.parametrize("row", range(len(SHARED_ROWS)))
def test_shared_rules(lib, entry, row):
    changes, want = SHARED_ROWS[row]
    expect(lib, entry, want, **changes)


def test_order_of_residual_and_source_checks(lib):
    """the exact-f32 form looks at the residual before the sources, the other two after them"""
    bad = dict(res=RES, res_stride=16, up0=8)
    expect(lib, RES3[0], RESIDUAL, **bad)
    expect(lib, RES3[1], UP, **bad)
    expect(lib, RES3[2], UP, **bad)


def test_f32_one_channel_layer(lib):
    f32 = RES3[0]
    one = dict(c0=1, stride0=1)
    expect(lib, f32, "the one-channel layer takes one full-resolution source", **dict(one, src1=SRC1))
    expect(lib, f32, "the one-channel layer takes one full-resolution source", **dict(one, up0=1))
    expect(lib, f32, "the one-channel layer takes one full-resolution source", **dict(one, stride0=2))
    expect(lib, f32, RESIDUAL + " a 32-channel-chunk layer", **dict(one, res=RES, res_stride=32))
    expect(lib, f32, ARGS, **dict(one, **TWO))                      # 1 + 32 channels
    expect(lib, f32, ARGS, **dict(one, c_out=30))
    for entry in RES3[1:]:                                           # the split forms have no one-channel layer
        expect(lib, entry, ARGS, **one)


def test_f16_row_offsets(lib):
    """buffer loads and stores address one row of the image with 32 bits"""
    big = dict(W=1 << 24)
    expect(lib, F16, ROW, **big)
    expect(lib, FMT, ROW, **big)
    expect(lib, RES3[0], ACCEPTED, **big)
    expect(lib, RES3[1], ACCEPTED, **big)
    expect(lib, RES3[0], ACCEPTED, W=(1 << 31) - 32, D=8, kz=3)      # 2^26 - 1 tiles per row, 2^29 tiles
    expect(lib, F16, ROW, W=(1 << 31) - 32, D=8, kz=3)
    expect(lib, F16, ACCEPTED, W=1 << 20)
    expect(lib, F16, ACCEPTED, W=1 << 20, c_out=256)
    expect(lib, F16, ROW, W=1 << 20, c_out=512)
    expect(lib, F16, ROW, W=1 << 20, c0=64, stride0=64)             # eleven source rows of 2^28 bytes
    expect(lib, F16, ACCEPTED, W=1 << 20, c0=64, stride0=64, up0=1)
    expect(lib, F16, ROW, W=1 << 20, res=RES, res_stride=512)
    expect(lib, F16, TILES, D=64, H=131072, W=131072, kz=3, c_out=128 * 128)     # the tile count comes first


def test_f16_range_flag(lib):
    for entry in (F16, FMT, DOT):
        head = dict(dotw=DOTW, dotp=DOTP) if entry == DOT else {}
        expect(lib, entry, ACCEPTED, flag=FLAG, **head)
        expect(lib, entry, ACCEPTED, flag=FLAG + 4, **head)
        expect(lib, entry, ARGS, flag=FLAG + 2, **head)
        expect(lib, entry, ARGS, flag=FLAG + 2, up0=8, **head)
        expect(lib, entry, None, flag=FLAG + 2, W=0, **head)


def test_f16_split16_rules(lib):
    head = dict(dotw=DOTW, dotp=DOTP)
    expect(lib, FMT, ACCEPTED)
    expect(lib, FMT, ACCEPTED, in_split=1)
    expect(lib, FMT, ACCEPTED, out_split=1)
    expect(lib, FMT, ACCEPTED, in_split=1, out_split=1, **TWO)
    expect(lib, FMT, ACCEPTED, in_split=1, **head)
    expect(lib, FMT, SPLIT, out_split=1, **head)
    expect(lib, FMT, SPLIT, out_split=1, dotw=DOTW)
    expect(lib, FMT, SPLIT, out_split=1, W=0, **head)                # before "nothing to do"
    expect(lib, FMT, None, W=0)
    expect(lib, FMT, SPLIT, out_split=1, act=2, **head)              # and before the arguments
    expect(lib, FMT, ACCEPTED, in_split=5)                           # the entry point reads its two flags as booleans
    expect(lib, FMT, ARGS, in_split=1, c0=48, stride0=48)
    expect(lib, FMT, UP, in_split=1, up0=1, W=7)


def test_f16_fused_head_rules(lib):
    head = dict(dotw=DOTW, dotp=DOTP)
    expect(lib, DOT, ACCEPTED, **head)
    expect(lib, FMT, ACCEPTED, **head)
    expect(lib, DOT, ACCEPTED, out=None, **head)                     # the head without the feature store
    expect(lib, FMT, ACCEPTED, out=None, in_split=1, **head)
    expect(lib, FMT, ARGS, out=None)
    expect(lib, FMT, ARGS, out=None, dotw=DOTW)
    rc, msg, _ = call(lib, DOT, dotw=DOTW)
    assert rc == -1 and msg.startswith("sd_conv3_f16x3_dot: head weights and partial-sum buffer required"), msg
    rc, msg, _ = call(lib, DOT, dotp=DOTP, W=0)
    assert rc == -1 and msg.startswith("sd_conv3_f16x3_dot: head weights and partial-sum buffer required"), msg
    expect(lib, FMT, HEAD, dotw=DOTW)
    expect(lib, FMT, HEAD, dotp=DOTP)
    expect(lib, FMT, HEAD, dotw=DOTW + 4, dotp=DOTP)
    expect(lib, FMT, HEAD, dotw=DOTW, dotp=DOTP + 2)
    expect(lib, FMT, ACCEPTED, dotw=DOTW, dotp=DOTP + 4)
    expect(lib, DOT, HEAD, W=1 << 22, c_out=512, **head)            # W * c_out = 2^31: the partial sums' row
    expect(lib, DOT, SOURCES, stride0=28, dotw=DOTW + 4, dotp=DOTP)                 # the sources come before the head
