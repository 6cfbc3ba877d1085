// Calls lsq::parse_job_args (lesseq_amd/csrc/lsq_jobargs.hpp) alone: no library, no environment, no device.  Built and run under
// AddressSanitizer + UBSan by tests/test_host_logic.py.  Every argv is handed over in an array of exactly argc words, so a look
// behind the last one is the sanitizer's to report.  Exit status 0 and "job args ok" when every case holds, else one line per
// broken expectation and exit status 1.
#include <cstdio>
#include <initializer_list>
#include <string>

#include "lsq_jobargs.hpp"

using lsq::ArgsResult;
using lsq::JobArgs;

static int g_broken = 0;
#define EXPECT(cond) do { if (!(cond)) { ++g_broken; fprintf(stderr, "%s:%d: expected %s\n", __FILE__, __LINE__, #cond); } } while (0)

typedef std::vector<std::string> Words;

static Words operator+(Words a, const Words &b) { a.insert(a.end(), b.begin(), b.end()); return a; }
static Words with(Words a, size_t at, const char *word) { a[at] = word; return a; }

static ArgsResult parse(bool solve, Words words, JobArgs &A) {
	static Words kept;                    // JobArgs points into the argv's words: they live until the next call
	kept = std::move(words);
	std::vector<const char *> argv;       // heap storage of exactly argc pointers
	for (const std::string &w : kept) argv.push_back(w.c_str());
	argv.shrink_to_fit();
	A = JobArgs();
	return lsq::parse_job_args(solve, (int)argv.size(), argv.data(), A);
}
static bool is(const char *a, const char *b) { return a && strcmp(a, b) == 0; }

// the fields of an accepted argv whose read files are `groups` copies of the group below
static void expect_accepted(bool solve, const JobArgs &A, int groups, bool fim, unsigned long B, unsigned long seed) {
	EXPECT(A.have_log_level && A.log_level == 2);
	EXPECT(is(A.annotation[0], "LH_GENE_TXT") && is(A.annotation[1], "toy.interval") && is(A.annotation[2], "UCSC_GENE2ISOFORM") && is(A.annotation[3], "toy.map"));
	EXPECT(A.gb == 0 && A.ge == 10);
	EXPECT(A.M() == groups && (int)A.fmts.size() == groups && (int)A.types.size() == groups && (int)A.lens.size() == groups && (int)A.paths.size() == groups);
	EXPECT((int)A.trb.size() == (solve ? groups : 0));
	for (int m = 0; m < A.M() && m < groups; ++m) {
		EXPECT(is(A.fmts[m], "MRF_SINGLE") && is(A.types[m], m ? "MEDIUM_READ" : "SHORT_READ") && A.lens[m] == (m ? 75u : 50u));
		if (solve) EXPECT(A.trb[m] == (m ? 1e6 : 650.0));
	}
	EXPECT(A.want_fim == fim && A.boot_B == B && A.boot_seed == seed);
}

int main() {
	const Words head = {"count", "2", "toy", "./", "LH_GENE_TXT", "toy.interval", "UCSC_GENE2ISOFORM", "toy.map", "0", "10"};
	const Words c1 = {"MRF_SINGLE", "SHORT_READ", "50", "toy.mrf"}, c2 = {"MRF_SINGLE", "MEDIUM_READ", "75", "more.mrf"};
	const Words s1 = c1 + Words{"650"}, s2 = c2 + Words{"1e6"};
	const Words count = head + c1, solve = head + s1;
	JobArgs A;

	// ---- accepted
	EXPECT(parse(false, count, A) == ArgsResult::Ok); expect_accepted(false, A, 1, false, 0, 0);
	EXPECT(is(A.paths[0], "toy.mrf"));
	EXPECT(parse(false, count + c2, A) == ArgsResult::Ok); expect_accepted(false, A, 2, false, 0, 0);
	EXPECT(is(A.paths[1], "more.mrf"));
	EXPECT(parse(true, solve, A) == ArgsResult::Ok); expect_accepted(true, A, 1, false, 0, 0);
	EXPECT(parse(true, solve + s2, A) == ArgsResult::Ok); expect_accepted(true, A, 2, false, 0, 0);
	EXPECT(parse(true, solve + Words{"--fim"}, A) == ArgsResult::Ok); expect_accepted(true, A, 1, true, 0, 0);
	EXPECT(parse(true, solve + Words{"--bootstrap", "7"}, A) == ArgsResult::Ok); expect_accepted(true, A, 1, false, 7, 0);
	EXPECT(parse(true, solve + Words{"--bootstrap", "4096", "--seed", "9"}, A) == ArgsResult::Ok); expect_accepted(true, A, 1, false, 4096, 9);
	EXPECT(parse(true, solve + Words{"--fim", "--bootstrap", "7", "--seed", "9"}, A) == ArgsResult::Ok); expect_accepted(true, A, 1, true, 7, 9);
	EXPECT(parse(true, solve + s2 + Words{"--fim", "--bootstrap", "1"}, A) == ArgsResult::Ok); expect_accepted(true, A, 2, true, 1, 0);
	// a path of this spelling below argv[15] is a path; so is `--fim` anywhere but last
	EXPECT(parse(true, with(solve, 13, "--bootstrap"), A) == ArgsResult::Ok); expect_accepted(true, A, 1, false, 0, 0);
	EXPECT(is(A.paths[0], "--bootstrap"));
	EXPECT(parse(true, with(solve, 13, "--fim"), A) == ArgsResult::Ok); expect_accepted(true, A, 1, false, 0, 0);
	EXPECT(is(A.paths[0], "--fim"));
	EXPECT(parse(false, with(count, 13, "--bootstrap"), A) == ArgsResult::Ok); expect_accepted(false, A, 1, false, 0, 0);
	// a negative log level passes the cast; so does a sign before a count
	EXPECT(parse(false, with(count, 1, "-1"), A) == ArgsResult::Ok && A.have_log_level && A.log_level == -1);
	EXPECT(parse(false, with(count, 9, "+10"), A) == ArgsResult::Ok && A.ge == 10);

	// ---- usage
	for (const Words &tail : {Words{"--bootstrap", "0"}, Words{"--bootstrap", "4097"}, Words{"--bootstrap", "x"}, Words{"--bootstrap"}, Words{"--bootstrap", "10", "--seed"},
	                          Words{"--bootstrap", "10", "--sed", "3"}, Words{"--bootstrap", "10", "--seed", "x"}, Words{"--bootstrap", "10", "--fim"},
	                          Words{"--bootstrap", "10", "--seed", "3", "--fim"}}) {
		EXPECT(parse(true, solve + tail, A) == ArgsResult::Usage);
		EXPECT(!A.have_log_level);          // decided before the log level is read
	}
	EXPECT(parse(false, head, A) == ArgsResult::Usage && !A.have_log_level);
	EXPECT(parse(true, count, A) == ArgsResult::Usage && !A.have_log_level);          // solve with count's group: too few words
	EXPECT(parse(true, Words{"solve"}, A) == ArgsResult::Usage);
	// count knows neither extension: the word starts an incomplete file group, after the log level was read
	EXPECT(parse(false, count + Words{"--fim"}, A) == ArgsResult::Usage && A.have_log_level && A.log_level == 2);
	EXPECT(parse(false, count + Words{"--bootstrap", "7"}, A) == ArgsResult::Usage && A.have_log_level);
	EXPECT(parse(true, solve + c2, A) == ArgsResult::Usage && A.have_log_level);

	// ---- the log level fails the cast; numbers that fail it, in the reference's order
	EXPECT(parse(false, with(count, 1, "abc"), A) == ArgsResult::Abort && !A.have_log_level);
	EXPECT(parse(false, with(count, 1, ""), A) == ArgsResult::Abort);
	EXPECT(parse(false, with(with(count, 1, "abc"), 8, "abc"), A) == ArgsResult::Abort);
	EXPECT(parse(false, with(count, 8, "abc"), A) == ArgsResult::BadNumber && A.have_log_level && A.log_level == 2);
	EXPECT(parse(false, with(count, 9, "1.5"), A) == ArgsResult::BadNumber);
	EXPECT(parse(false, with(count, 12, "fifty"), A) == ArgsResult::BadNumber);
	EXPECT(parse(true, with(solve, 14, "abc"), A) == ArgsResult::BadNumber);
	EXPECT(parse(true, with(solve, 14, " 650"), A) == ArgsResult::BadNumber);
	EXPECT(parse(false, with(count, 12, "fifty") + Words{"x"}, A) == ArgsResult::BadNumber);          // the first thing wrong speaks
	EXPECT(parse(false, with(count, 12, "99999999999999999999999"), A) == ArgsResult::BadNumber);

	// ---- too many read files: decided last
	Words many = head, many_solve = head;
	for (int m = 0; m < LSQ_MAX_METHODS; ++m) { many = many + c1; many_solve = many_solve + s1; }
	EXPECT(parse(false, many, A) == ArgsResult::Ok && A.M() == LSQ_MAX_METHODS);
	EXPECT(parse(false, many + c1, A) == ArgsResult::TooManyFiles && A.M() == LSQ_MAX_METHODS + 1);
	EXPECT(parse(true, many_solve + s1, A) == ArgsResult::TooManyFiles);
	EXPECT(parse(false, many + with(c1, 2, "fifty"), A) == ArgsResult::BadNumber);

	if (g_broken) return 1;
	printf("job args ok\n");
	return 0;
}
