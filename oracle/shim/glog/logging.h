// Stand-in for glog when the checker compiles the reference's tracking_loop_filter.cc on its own (oracle/Makefile,
// _ref/libref_loop.so): LOG(x) << ... compiles and writes nowhere.
#pragma once
struct OracleNullLog { template <class T> OracleNullLog& operator<<(const T&) { return *this; } };
#define LOG(severity) OracleNullLog()
