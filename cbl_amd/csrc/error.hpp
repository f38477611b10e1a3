// error.hpp — what every layer of libcblx throws: a code of include/cblx.h and a text. No HIP in here (the host-only headers throw it too).
#pragma once
#include <stdexcept>
#include <string>

namespace cblx {
struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};
}  // namespace cblx
