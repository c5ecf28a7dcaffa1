"""CPU tests (no GPU) of the signal generator's C ABI (gc_signal_generator_*, gc_siggen_*): the declarations compile as C and C++,
the struct mirrors have the library's sizes, every argument is checked before anything needs a device, and a machine without a
GPU fails loudly."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["gc_signal_generator_create", "gc_signal_generator_destroy", "gc_signal_generator_generate", "gc_signal_generator_info",
    "gc_signal_generator_set_output_scale", "gc_signal_generator_output_info", "gc_signal_generator_plan", "gc_siggen_reference_satellite",
    "gc_siggen_component_size", "gc_siggen_sat_size", "gc_siggen_conf_size"]


def test_header_with_signal_generator_compiles_as_c_and_cpp(tmp_path):
    body = ('#include "gnsscorr.h"\n'
            'static gc_status (*const f_create)(gc_ctx*, const gc_siggen_conf*, gc_stream*, gc_signal_generator**) = gc_signal_generator_create;\n'
            'static gc_status (*const f_generate)(gc_signal_generator*, uint64_t, uint64_t*) = gc_signal_generator_generate;\n'
            'static gc_status (*const f_info)(gc_signal_generator*, uint64_t*) = gc_signal_generator_info;\n'
            'static gc_status (*const f_scale)(gc_signal_generator*, float) = gc_signal_generator_set_output_scale;\n'
            'static gc_status (*const f_out)(gc_signal_generator*, int32_t*, float*, uint64_t*) = gc_signal_generator_output_info;\n'
            'static gc_status (*const f_destroy)(gc_signal_generator*) = gc_signal_generator_destroy;\n'
            'static gc_status (*const f_plan)(const gc_siggen_sat*, double, uint64_t*, uint64_t*, uint64_t*, uint64_t*) = gc_signal_generator_plan;\n'
            'int main(void){ gc_siggen_conf c; c.n_sats = GC_SIGGEN_MAX_SATS; (void)c; (void)f_create; (void)f_generate; (void)f_info; (void)f_scale;\n'
            ' (void)f_out; (void)f_destroy; (void)f_plan;\n'
            ' return sizeof(gc_siggen_component) == 40 && sizeof(gc_siggen_sat) == 128 && sizeof(gc_siggen_conf) == 48 && GC_SIGGEN_MAX_TABLE == 49104 ? 0 : 1; }\n')
    for cc, std, name in (("gcc", "-std=c99", "t.c"), ("g++", "-std=c++11", "t.cpp")):
        src = tmp_path / name
        src.write_text(body)
        exe = str(tmp_path / (name + ".exe"))
        subprocess.check_call([cc, std, "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", exe + ".o"])


def test_library_exports_the_signal_generator_symbols_and_struct_sizes():
    import gnsscorr
    lib = gnsscorr.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), "libgnsscorr.so does not export %s" % name
        assert name in gnsscorr.API, name
    assert lib.gc_siggen_component_size() == C.sizeof(gnsscorr.SiggenComponent) == 40
    assert lib.gc_siggen_sat_size() == C.sizeof(gnsscorr.SiggenSat) == 128
    assert lib.gc_siggen_conf_size() == C.sizeof(gnsscorr.SiggenConf) == 48
    assert hasattr(gnsscorr, "SignalGenerator") and hasattr(gnsscorr, "siggen_plan") and hasattr(gnsscorr, "siggen_reference_satellite")
    assert gnsscorr.SignalGenerator._C == "gc_signal_generator" and issubclass(gnsscorr.SignalGenerator, gnsscorr._RingStage)


TABLE = np.ones(49104 + 1, np.float32)
SECONDARY = np.ones(101, np.int8)


def _sat(table_len=1023, n_components=1, code_periods_per_sample=1.0 / 4000.0, code_phase0_periods=0.0, doppler_hz=0.0, amplitude=1.0,
        carrier_phase0_turns=0.0, secondary_len=0, axis=0, gain=1.0, table=TABLE, secondary=SECONDARY):
    import gnsscorr
    s = gnsscorr.SiggenSat()
    s.doppler_hz, s.carrier_phase0_turns, s.code_phase0_periods, s.code_periods_per_sample = doppler_hz, carrier_phase0_turns, code_phase0_periods, code_periods_per_sample
    s.amplitude, s.table_len, s.n_components = amplitude, table_len, n_components
    for c in range(2):
        k = s.comp[c]
        k.table = None if table is None else table.ctypes.data_as(C.POINTER(C.c_float))
        k.secondary = None if secondary is None else secondary.ctypes.data_as(C.POINTER(C.c_int8))
        k.secondary_len, k.axis, k.gain = secondary_len, axis, gain
    return s


def _create(sats, n_sats=None, fs_hz=4e6, noise_sigma=0.0, placement=0, conf=True):
    import gnsscorr
    lib = gnsscorr.load_library()
    arr = (gnsscorr.SiggenSat * max(1, len(sats)))(*sats)
    c = gnsscorr.SiggenConf(fs_hz, noise_sigma, 0, 0, len(sats) if n_sats is None else n_sats, placement, arr)
    out = C.c_void_p()
    st = lib.gc_signal_generator_create(None, C.byref(c) if conf else None, None, C.byref(out))
    assert not out.value
    return st, lib.gc_last_error().decode()


BAD_TABLE = np.ones(16, np.float32)
BAD_TABLE[5] = np.inf
BAD_SECONDARY = np.array([1, -1, 0, 1], np.int8)


@pytest.mark.parametrize("make, word", [
    (lambda: _create([], n_sats=0), "0 satellites"),
    (lambda: _create([_sat()] * 33), "33 satellites"),
    (lambda: _create([_sat(table_len=0)]), "table_len 0"),
    (lambda: _create([_sat(table_len=49105)]), "table_len 49105"),
    (lambda: _create([_sat(n_components=3)]), "3 components"),
    (lambda: _create([_sat(n_components=0)]), "0 components"),
    (lambda: _create([_sat(code_periods_per_sample=0.0)]), "code_periods_per_sample 0 is outside (0, 1)"),
    (lambda: _create([_sat(code_periods_per_sample=1.0)]), "code_periods_per_sample 1 is outside (0, 1)"),
    (lambda: _create([_sat(code_periods_per_sample=-0.25)]), "code_periods_per_sample -0.25 is outside (0, 1)"),
    (lambda: _create([_sat(code_periods_per_sample=float("nan"))]), "code_periods_per_sample"),
    (lambda: _create([_sat(code_periods_per_sample=1e-30)]), "rounds to a step of 0"),
    (lambda: _create([_sat(code_phase0_periods=1.0)]), "code_phase0_periods 1 is outside [0, 1)"),
    (lambda: _create([_sat(code_phase0_periods=float("nan"))]), "code_phase0_periods"),
    (lambda: _create([_sat(doppler_hz=float("nan"))]), "doppler_hz is not finite"),
    (lambda: _create([_sat(carrier_phase0_turns=float("inf"))]), "carrier_phase0_turns is not finite"),
    (lambda: _create([_sat(amplitude=float("nan"))]), "amplitude of satellite 0 is not finite"),
    (lambda: _create([_sat(), _sat(secondary_len=101)]), "satellite 1 has secondary_len 101"),
    (lambda: _create([_sat(secondary_len=4, secondary=None)]), "NULL secondary code"),
    (lambda: _create([_sat(secondary_len=4, secondary=BAD_SECONDARY)]), "symbol 2 of the secondary code"),
    (lambda: _create([_sat(table=None)]), "NULL table"),
    (lambda: _create([_sat(table_len=16, table=BAD_TABLE)]), "entry 5 of the table"),
    (lambda: _create([_sat(axis=2)]), "axis 2"),
    (lambda: _create([_sat(gain=float("nan"))]), "gain of component 0"),
    (lambda: _create([_sat()], fs_hz=0.0), "fs_hz must be finite and positive"),
    (lambda: _create([_sat()], fs_hz=float("nan")), "fs_hz must be finite and positive"),
    (lambda: _create([_sat()], noise_sigma=-1.0), "noise_sigma"),
    (lambda: _create([_sat()], noise_sigma=float("nan")), "noise_sigma"),
    (lambda: _create([_sat()], placement=3), "unknown table placement 3"),
    (lambda: _create([_sat(table_len=10230, n_components=2)], placement=2), "do not fit in LDS"),
    (lambda: _create([_sat()], conf=False), "NULL configuration"),
])
def test_every_argument_is_checked_before_any_device_call(make, word):
    """No context exists on a machine without a GPU: every limit must be reported with NULL handles, with nothing created."""
    import gnsscorr
    st, msg = make()
    assert st == gnsscorr.GC_ERR_INVALID and word in msg and msg.startswith("gc_signal_generator_create: "), msg


def test_configurations_at_the_limits_get_as_far_as_the_handles():
    import gnsscorr
    lib = gnsscorr.load_library()
    for sats, kw in (([_sat()], {}), ([_sat()] * 32, {}), ([_sat(table_len=49104, n_components=2, secondary_len=100)], {}),
            ([_sat(table_len=1, code_periods_per_sample=0.999, code_phase0_periods=0.999, doppler_hz=-1e9)], dict(noise_sigma=3.0)),
            ([_sat(table_len=7680, n_components=2)], dict(placement=2))):
        st, msg = _create(sats, **kw)
        assert st == gnsscorr.GC_ERR_INVALID and "NULL argument" in msg, msg
    assert lib.gc_signal_generator_generate(None, 5, None) == gnsscorr.GC_ERR_INVALID
    assert lib.gc_signal_generator_info(None, None) == gnsscorr.GC_ERR_INVALID
    assert lib.gc_signal_generator_output_info(None, None, None, None) == gnsscorr.GC_ERR_INVALID
    assert lib.gc_signal_generator_set_output_scale(None, C.c_float(0.0)) == gnsscorr.GC_ERR_INVALID
    assert "not finite and positive" in lib.gc_last_error().decode()
    assert lib.gc_signal_generator_set_output_scale(None, C.c_float(2.0)) == gnsscorr.GC_ERR_INVALID
    assert "NULL handle" in lib.gc_last_error().decode()
    assert lib.gc_signal_generator_destroy(None) == gnsscorr.GC_OK
    assert lib.gc_signal_generator_plan(None, 4e6, None, None, None, None) == gnsscorr.GC_ERR_INVALID
    s = _sat()
    assert lib.gc_signal_generator_plan(C.byref(s), 4e6, None, None, None, None) == gnsscorr.GC_OK
    assert lib.gc_signal_generator_plan(C.byref(s), 0.0, None, None, None, None) == gnsscorr.GC_ERR_INVALID


def test_no_gpu_means_loud_failure_for_create():
    """Where there is no usable GPU there is no context, hence no ring and no generator: nothing falls back to the host."""
    import gnsscorr
    if gnsscorr.device_count() == 0:
        with pytest.raises(gnsscorr.GnsscorrError) as e:
            gnsscorr.Context(0)
        assert e.value.status == gnsscorr.GC_ERR_NO_DEVICE
    sat = gnsscorr.SiggenSatellite(0.0, 1.0 / 4000.0, [dict(table=np.ones(1023, np.float32))])

    class NoHandle:
        _h = None
    with pytest.raises(gnsscorr.GnsscorrError) as e:
        gnsscorr.SignalGenerator(NoHandle(), NoHandle(), 4e6, [sat])
    assert e.value.status == gnsscorr.GC_ERR_INVALID and "NULL argument" in str(e.value)
