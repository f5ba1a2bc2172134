// thread-local "last error" shared by the C-ABI translation units, and the one mapping of a C++ exception to an error code
#pragma once
#include <new>
#include <stdexcept>

#include "../../include/ds2i_hip.h"

int ds2i_set_error(int code, const char* msg);
const char* ds2i_get_error();

// The body of a C-ABI entry point (or of a helper that returns its error code) between DS2I_TRY and DS2I_CATCH: no exception crosses
// the ABI. std::invalid_argument is what the host builders throw for a bad argument ("List must be nonempty"); everything else they
// throw is about an image or a sequence that does not hold together.
#define DS2I_TRY try {
#define DS2I_CATCH                                                                                   \
    } catch (std::bad_alloc const&) { return ds2i_set_error(DS2I_ENOMEM, "out of host memory"); }   \
    catch (std::invalid_argument const& e) { return ds2i_set_error(DS2I_EINVAL, e.what()); }         \
    catch (std::exception const& e) { return ds2i_set_error(DS2I_EFORMAT, e.what()); }
