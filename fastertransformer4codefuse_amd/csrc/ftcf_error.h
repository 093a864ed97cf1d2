// The engine's exception and argument check, without HIP: host-only headers (batcher_sched.h) and their check programs use them too.
#pragma once
#include <stdexcept>
#include <string>

namespace ftcf {

struct Error : public std::runtime_error {
    int code;
    Error(int c, const std::string& s): std::runtime_error(s), code(c) {}
};

#define FTCF_CHECK_ARG(cond, msg)                                                                                      \
    do {                                                                                                               \
        if (!(cond)) {                                                                                                 \
            throw ::ftcf::Error(-1, std::string("invalid argument: ") + (msg) + " [" #cond "]");                       \
        }                                                                                                              \
    } while (0)

}  // namespace ftcf
