// rkf_weights.h — the Fehlberg weights of rkf45_step's fifth-order result (CH) and of its
// error estimate (CT), runge_kutta.rs:62-84.  Shared by the device (geodesic_rkf.h) and the
// host check of the sums without their zero-weight k2 terms
// (tests/native/rkf_zero_terms_check.cpp).
#pragma once

namespace grt {

constexpr double CH1 = 47.0 / 450.0, CH2 = 0.0, CH3 = 12.0 / 25.0, CH4 = 32.0 / 225.0,
                 CH5 = 1.0 / 30.0, CH6 = 6.0 / 25.0;
constexpr double CT1 = 1.0 / 150.0, CT2 = 0.0, CT3 = -3.0 / 100.0, CT4 = 16.0 / 75.0,
                 CT5 = 1.0 / 20.0, CT6 = -6.0 / 25.0;

}  // namespace grt
