// host_util.h -- what every host translation unit of the C-ABI shares (both functions are defined in corb_orb.cpp): the calling thread's error message, the
// device selection, and the check that turns a failed HIP call into that message and CORB_ERR_HIP.  Host code only.
#pragma once
#include "corb_internal.h"

void corb_set_error(const char* fmt, ...);
int corb_select_device(int device);
#define HIPCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { corb_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); return CORB_ERR_HIP; } } while (0)
