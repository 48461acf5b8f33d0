// module_cli.h -- internal: the command-line plumbing the module mains share (mdf_modules.cpp, where it is defined, and tool_modules.cpp):
// the common flags, the argument loop and the log set-up.
#pragma once
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "module_log.h"

namespace tkmod {

struct Common {
    std::string input, output, verbosity = "INFO", log_file = "stderr";
    long long seed = 42;
    std::vector<int> devices{0};
    uint64_t batch_bytes = 64ull << 20;          // truncate: MDF text per batch
    uint64_t slice_molecules = 2000000;          // pcr: output molecules per slice of templates
    bool help = false;
};

// The argument loop of every module: "--flag=value" split in two, then own(o, v) for each argument o with the one behind it (v, or null) --
// the module's own flags, which come first (random-wgs refuses some of the common ones) -- then the common flags.  The texts are cxxopts'.
enum { NOT_MINE = 0, TOOK_FLAG = 1, TOOK_VALUE = 2, REFUSED = -1 /* own() has said why */, NO_SUCH = -2, MALFORMED = -3 };
bool parse_args(int argc, char** argv, Common& c, const std::function<int(const std::string&, const char*)>& own);

// --verbosity and --log-file applied to log; false: said why on stderr
bool open_log(const Common& c, const char* module, Logger& log);

}  // namespace tkmod
