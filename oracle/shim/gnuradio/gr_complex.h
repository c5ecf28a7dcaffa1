// Stand-in for GNU Radio's header when the checker compiles the reference's discriminators and lock detectors on their own
// (oracle/Makefile, _ref/libref_loop.so): gr_complex is a complex float.
#pragma once
#include <complex>
typedef std::complex<float> gr_complex;
