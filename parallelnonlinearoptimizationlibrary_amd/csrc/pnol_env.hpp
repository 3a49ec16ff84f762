// pnol_env.hpp -- the one reader of the PNOL_* tuning switches (internal).  Each call reads the
// environment: a switch read once per process sits in a function-local static at its call.
// (runtime.cpp's strict env_int, for the MPI launcher's variables, is a different parse.)
#pragma once

#include <cstdlib>
#include <cstring>

namespace pnol {

// an integer switch: atoi of its value, dflt when unset
inline int env_atoi(const char* name, int dflt) {
    const char* e = std::getenv(name);
    return e ? std::atoi(e) : dflt;
}
// on unless set to 0
inline bool env_default_on(const char* name) { return env_atoi(name, 1) != 0; }
// a named choice: the value equals s (if_unset when the switch is not set)
inline bool env_equals(const char* name, const char* s, bool if_unset = false) {
    const char* e = std::getenv(name);
    return e ? std::strcmp(e, s) == 0 : if_unset;
}

}  // namespace pnol
