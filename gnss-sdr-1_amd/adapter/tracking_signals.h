/*!
 * \file tracking_signals.h
 * \brief What the tracking blocks and adapters of this directory know about a signal, written once: the table of the seven signals
 * of dll_pll_veml_tracking (one row per signal: the constants of the block's constructor, dll_pll_veml_tracking.cc:113-336, and the
 * defaults of its reference adapter), the replica generators that serve them (trk_generate_replicas), and the GPS L1 / GLONASS
 * L1 / L2 C/A constants of the GLONASS and carrier-aided blocks.
 */
#ifndef GNSSCORR_TRACKING_SIGNALS_H_
#define GNSSCORR_TRACKING_SIGNALS_H_

#include "gnsscorr.h"
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace gnsscorr
{
//! index of a row of trk_signal_table()
enum class TrkSignal
{
    GPS_L1_CA,
    GALILEO_E1,
    BEIDOU_B1I,
    GPS_L2_M,
    GPS_L5,
    GALILEO_E5A,
    BEIDOU_B3I
};

struct TrkSignalInfo
{
    char system;
    const char* signal;
    // the block's constructor (dll_pll_veml_tracking.cc:113-336)
    double carrier_freq_hz, code_period_s, code_chip_rate_hz;
    uint32_t code_length_chips, code_samples_per_chip;
    bool veml, has_pilot, interchange_iq_with_pilot;
    int32_t correlation_length_ms;
    // what differs between the reference's adapters: name, default loop settings, lock thresholds, extension rule
    const char* implementation;
    float pll_bw_hz, dll_bw_hz, pll_bw_narrow_hz, dll_bw_narrow_hz;
    float early_late_space_chips, early_late_space_narrow_chips;
    int cn0_min;
    double carrier_lock_th;
    int max_extension_data;  //!< longest integration (symbols) on the data component; 0: only with the pilot
};

constexpr int kTrkSignals = 7;

inline const TrkSignalInfo* trk_signal_table()
{
    static const TrkSignalInfo t[kTrkSignals] = {
        {'G', "1C", 1575.42e6, 0.001, 1.023e6, 1023, 1, false, false, false, 1, "GPS_L1_CA_DLL_PLL_Tracking_HIP", 50.0f, 2.0f, 20.0f, 2.0f, 0.5f, 0.5f, 30, 0.80, 20},
        // sinBOC(1,1) replica, 2 samples per chip; E1-B and E1-C are in anti-phase: no I/Q interchange with the pilot
        {'E', "1B", 1575.42e6, 0.004, 1.023e6, 4092, 2, true, true, false, 4, "Galileo_E1_DLL_PLL_VEML_Tracking_HIP", 5.0f, 0.5f, 2.0f, 0.25f, 0.15f, 0.15f, 25, 0.85, 0},
        {'C', "B1", 1.561098e9, 0.001, 2.046e6, 2046, 1, false, false, false, 1, "BEIDOU_B1I_DLL_PLL_Tracking_HIP", 50.0f, 2.0f, 20.0f, 2.0f, 0.5f, 0.5f, 25, 0.85, 20},
        // gps_l2_m_dll_pll_tracking.cc:47-170: one 20 ms code per symbol, extension forced to 1
        {'G', "2S", 1.22760e9, 0.02, 0.5115e6, 10230, 1, false, false, false, 20, "GPS_L2_M_DLL_PLL_Tracking_HIP", 2.0f, 0.75f, 2.0f, 0.75f, 0.5f, 0.5f, 25, 0.85, 1},
        // gps_l5_dll_pll_tracking.cc:47-200: data component L5I (NH10) or pilot L5Q (NH20), in quadrature
        {'G', "L5", 1.17645e9, 0.001, 10.23e6, 10230, 1, false, true, true, 1, "GPS_L5_DLL_PLL_Tracking_HIP", 50.0f, 2.0f, 2.0f, 0.25f, 0.5f, 0.15f, 25, 0.75, 10},
        // galileo_e5a_dll_pll_tracking.cc:47-200: data component E5a-I (CS20) or pilot E5a-Q (CS100 per PRN), in quadrature
        {'E', "5X", 1.17645e9, 0.001, 1.023e7, 10230, 1, false, true, true, 1, "Galileo_E5a_DLL_PLL_Tracking_HIP", 20.0f, 20.0f, 5.0f, 2.0f, 0.5f, 0.15f, 25, 0.85, 20},
        // beidou_b3i_dll_pll_tracking.cc:47-190
        {'C', "B3", 1.268520e9, 0.001, 10.23e6, 10230, 1, false, false, false, 1, "BEIDOU_B3I_DLL_PLL_Tracking_HIP", 50.0f, 2.0f, 20.0f, 2.0f, 0.5f, 0.5f, 25, 0.85, 20}};
    return t;
}

inline const TrkSignalInfo& trk_signal(TrkSignal s) { return trk_signal_table()[static_cast<int>(s)]; }

//! the row of (system, signal), or NULL: not a signal of dll_pll_veml_tracking
inline const TrkSignalInfo* trk_signal_find(char system, const std::string& signal)
{
    for (int i = 0; i < kTrkSignals; i++)
        if (trk_signal_table()[i].system == system && signal == trk_signal_table()[i].signal) return &trk_signal_table()[i];
    return nullptr;
}

/*! The replica a tracking loop runs on (start_tracking, dll_pll_veml_tracking.cc:566-705): `code` receives code_length_chips *
 *  code_samples_per_chip floats -- the pilot component's with `pilot` (L5Q, E1-C, E5a-Q), else the data component's.  data_code
 *  receives the data component's replica when `pilot` is set and the pointer is not NULL, and is left alone otherwise.  Returns the
 *  first generator status that is not GC_OK (e.g. a PRN the signal does not have). */
inline gc_status trk_generate_replicas(char system, const char* signal, uint32_t prn, bool pilot, float* code, float* data_code)
{
    const TrkSignalInfo* sig = trk_signal_find(system, signal);
    if (sig == nullptr) return GC_ERR_INVALID;
    float* data = pilot ? data_code : nullptr;
    gc_status st = GC_OK, st_data = GC_OK;
    switch (static_cast<TrkSignal>(sig - trk_signal_table()))
        {
        case TrkSignal::GPS_L1_CA:
            return gc_gps_l1_ca_code_gen_float(code, static_cast<int32_t>(prn), 0);
        case TrkSignal::GPS_L2_M:
            return gc_gps_l2c_m_code_gen_float(code, prn);
        case TrkSignal::BEIDOU_B1I:
            return gc_beidou_b1i_code_gen_float(code, static_cast<int32_t>(prn), 0);
        case TrkSignal::BEIDOU_B3I:
            return gc_beidou_b3i_code_gen_float(code, static_cast<int32_t>(prn), 0);
        case TrkSignal::GPS_L5:
            st = pilot ? gc_gps_l5q_code_gen_float(code, prn) : gc_gps_l5i_code_gen_float(code, prn);
            if (data) st_data = gc_gps_l5i_code_gen_float(data, prn);
            break;
        case TrkSignal::GALILEO_E1:
            st = gc_galileo_e1_code_gen_sinboc11_float(code, pilot ? "1C" : "1B", prn);
            if (data) st_data = gc_galileo_e1_code_gen_sinboc11_float(data, "1B", prn);
            break;
        case TrkSignal::GALILEO_E5A:
            {
                // the complex primary code holds E5a-I in the real and E5a-Q in the imaginary part (:606-626)
                std::vector<float> aux(2 * sig->code_length_chips);
                st = gc_galileo_e5_a_code_gen_complex_primary(aux.data(), static_cast<int32_t>(prn), "5X");
                for (uint32_t i = 0; i < sig->code_length_chips; i++)
                    {
                        code[i] = pilot ? aux[2 * i + 1] : aux[2 * i];
                        if (data) data[i] = aux[2 * i];
                    }
                break;
            }
        }
    return st != GC_OK ? st : st_data;
}

//! GPS_L1_FREQ_HZ, GPS_L1_CA_CODE_RATE_CPS, GPS_L1_CA_CODE_LENGTH_CHIPS for the blocks that are not table-driven
inline const TrkSignalInfo& gps_l1_ca() { return trk_signal(TrkSignal::GPS_L1_CA); }

//! GLONASS L1 / L2 C/A (GLONASS_L1_L2_CA.h:84-97): band centre, FDMA channel spacing, the code both bands share
struct GlonassBand
{
    double freq_hz, dfreq_hz;
    const char* implementation;      //!< the host-loop adapter's name
    const char* implementation_dev;  //!< the device-loop adapter's
};
constexpr double kGlonassCaCodeRateHz = 0.511e6;  // GLONASS_L1_CA_CODE_RATE_HZ (L2 C/A: the same)
constexpr int kGlonassCaCodeLengthChips = 511;
inline GlonassBand glonass_band(int band)
{
    return band == 2 ? GlonassBand{1.246e9, 0.4375e6, "GLONASS_L2_CA_DLL_PLL_Tracking_HIP", "GLONASS_L2_CA_DLL_PLL_Tracking_Dev_HIP"}
                     : GlonassBand{1.602e9, 0.5625e6, "GLONASS_L1_CA_DLL_PLL_Tracking_HIP", "GLONASS_L1_CA_DLL_PLL_Tracking_Dev_HIP"};
}

//! what a GLONASS block or group on the device loop is given
struct GlonassTrkConf
{
    int band = 1;
    int64_t fs_in = 0;
    uint32_t vector_length = 0;
    float pll_bw_hz = 50.0f, dll_bw_hz = 2.0f, early_late_space_chips = 0.5f;
    int cn0_samples = 20, cn0_min = 25, max_lock_fail = 50;
    double carrier_lock_th = 0.85;
};
}  // namespace gnsscorr

#endif  // GNSSCORR_TRACKING_SIGNALS_H_
