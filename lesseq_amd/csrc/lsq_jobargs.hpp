// The argv of count and solve (count/count.cpp:88-129, solve/solve.cpp:102-146) and the numeric casts of every executable.
// std and the ABI header's constants only -- no environment, no log, no device: tests/host/job_args_check.cpp calls it alone.
#pragma once

#include <cctype>
#include <cerrno>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/lesseq_hip.h"

namespace lsq {

// boost::lexical_cast<long / unsigned long / double>: the whole word, or nothing
inline bool cast_digits(const char *s) {
	if (!*s) return false;
	size_t i = (s[0] == '+' || s[0] == '-') ? 1 : 0;
	if (!s[i]) return false;
	for (size_t j = i; s[j]; ++j) if (s[j] < '0' || s[j] > '9') return false;
	return true;
}
inline bool cast_long(const char *s, long &out) {
	if (!cast_digits(s)) return false;
	errno = 0; char *e; long v = strtol(s, &e, 10);
	if (errno == ERANGE || *e) return false;
	out = v; return true;
}
inline bool cast_ulong(const char *s, unsigned long &out) {
	if (!cast_digits(s)) return false;
	errno = 0; char *e; unsigned long v = strtoul(s, &e, 10);
	if (errno == ERANGE || *e) return false;
	out = v; return true;
}
inline bool cast_double(const char *s, double &out) {
	if (!*s || isspace((unsigned char)*s)) return false;
	char *e; double v = strtod(s, &e);
	if (e == s || *e) return false;
	out = v; return true;
}

struct JobArgs {
	bool have_log_level = false;      // argv[1] passed the cast: log_level holds, whatever the result (the log level is set before anything else is cast)
	int log_level = 0;
	const char *annotation[4] = {nullptr, nullptr, nullptr, nullptr};      // isoform_format isoforms_path g2i_format g2i_path
	unsigned long gb = 0, ge = 0;
	std::vector<const char *> fmts, types, paths;      // per read file
	std::vector<uint64_t> lens;
	std::vector<double> trb;                           // solve: total_read_bases
	// Extensions (not in the reference, whose fim.h is dead code): `solve ... --fim` after the last read file appends, behind
	// the table, one `#fim` line per event and read file with fim.h's two variance estimates and the expected Fisher
	// information matrix (lsq_fim; parity unpinned), and `solve ... [--fim] --bootstrap B [--seed S]` appends, behind the table
	// and the `#fim` lines, one `#boot` line per event form with the summaries of B read-bootstrap replicates of theta
	// (lsq_bootstrap); seed 0 unless given.  The table itself does not change.
	bool want_fim = false;
	unsigned long boot_B = 0, boot_seed = 0;
	int M() const { return (int)paths.size(); }
};

enum class ArgsResult {
	Ok,
	Usage,             // exit 1 with the usage text
	Abort,             // the log level fails the cast, outside the reference's try block (count/count.cpp:99): exit 134, no log line
	BadNumber,         // exit 1 with the Lexical_cast line
	TooManyFiles       // more than LSQ_MAX_METHODS read files: exit 2
};

// The first thing wrong with the argv, in the reference's order.  `--bootstrap` is looked for from argv[15] on only (below that a
// word of this spelling is a path or a name), with exactly 1 or 3 words behind it; `--fim` only as the last word before it.
inline ArgsResult parse_job_args(bool solve, int argc, const char *const *argv, JobArgs &A) {
	const int per = solve ? 5 : 4;
	if (solve) {
		int at = -1;
		for (int i = 15; i < argc && at < 0; ++i) if (strcmp(argv[i], "--bootstrap") == 0) at = i;
		if (at >= 0) {
			const int rest = argc - at;
			if (rest != 2 && rest != 4) return ArgsResult::Usage;
			if (!cast_ulong(argv[at + 1], A.boot_B) || A.boot_B < 1 || A.boot_B > 4096) return ArgsResult::Usage;
			if (rest == 4 && (strcmp(argv[at + 2], "--seed") != 0 || !cast_ulong(argv[at + 3], A.boot_seed))) return ArgsResult::Usage;
			argc = at;
		}
	}
	if (solve && argc > 15 && strcmp(argv[argc - 1], "--fim") == 0) { A.want_fim = true; --argc; }
	if (argc < (solve ? 15 : 14)) return ArgsResult::Usage;
	long lvl;
	if (!cast_long(argv[1], lvl)) return ArgsResult::Abort;
	A.log_level = (int)lvl; A.have_log_level = true;
	for (int k = 0; k < 4; ++k) A.annotation[k] = argv[4 + k];
	if (!cast_ulong(argv[8], A.gb) || !cast_ulong(argv[9], A.ge)) return ArgsResult::BadNumber;
	for (int i = 10; i < argc;) {
		if (argc - i < per) return ArgsResult::Usage;
		A.fmts.push_back(argv[i++]);
		A.types.push_back(argv[i++]);
		unsigned long L;
		if (!cast_ulong(argv[i++], L)) return ArgsResult::BadNumber;
		A.lens.push_back(L);
		A.paths.push_back(argv[i++]);
		if (solve) { double v; if (!cast_double(argv[i++], v)) return ArgsResult::BadNumber; A.trb.push_back(v); }
	}
	return A.M() > LSQ_MAX_METHODS ? ArgsResult::TooManyFiles : ArgsResult::Ok;
}

} // namespace lsq
