// t41_sdr_amd/csrc/last_error.hpp -- the one error message of the library: t41rx_last_error() returns it for the
// calling thread, and every failing t41rx_* and t41tx_* entry point sets it (rx_host.cpp defines it).
#pragma once
#include <string>

namespace t41 {

// stores msg as the calling thread's last error and returns code
int fail(int code, const std::string &msg);

}  // namespace t41
