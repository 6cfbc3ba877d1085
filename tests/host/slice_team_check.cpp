// Drives lsq::SliceTeam (lesseq_amd/csrc/lsq_team.hpp) with fake stage bodies: no device, no library.  Built and run under
// ThreadSanitizer and under AddressSanitizer + UBSan by tests/test_host_logic.py; every case is repeated to vary the schedule.
// Exit status 0 and "slice team ok" when every case holds, else one line per broken expectation and exit status 1.
#include <atomic>
#include <cstdio>
#include <stdexcept>

#include "lsq_team.hpp"

using lsq::SliceTeam;

static int g_broken = 0;
#define EXPECT(cond) do { if (!(cond)) { ++g_broken; fprintf(stderr, "%s:%d (round %d): expected %s\n", __FILE__, __LINE__, round, #cond); } } while (0)

static const char *no_text() { return "status without a text"; }
static void jitter(int round, int r) { for (int i = (round * 7 + r * 3) % 5; i > 0; --i) std::this_thread::yield(); }

// two stages with a meeting after each; `stage(k, r)` is the fake body, and what every slice saw comes back in met[k][r]
template <class Stage>
static void two_stages(SliceTeam &team, int round, Stage &&stage, bool met[2][8], std::atomic<int> ran[2]) {
	team.run([&](int r) {
		for (int k = 0; k < 2; ++k) {
			if (k == 0 || met[0][r]) {
				jitter(round, r + k);
				team.guard(r, no_text, [&] { ++ran[k]; return stage(k, r); });
			}
			met[k][r] = team.meet(r);
		}
	});
}

int main() {
	const int ROUNDS = 300;
	for (int round = 0; round < ROUNDS; ++round) {
		{       // one slice: nothing to wait for
			SliceTeam team(1);
			bool met[2][8] = {}; std::atomic<int> ran[2] = {{0}, {0}};
			two_stages(team, round, [](int, int) { return 0; }, met, ran);
			EXPECT(met[0][0] && met[1][0] && ran[0] == 1 && ran[1] == 1 && team.first_failure() == -1 && team.status(0) == LSQ_OK);
		}
		{       // four slices, all well over two meetings
			SliceTeam team(4);
			bool met[2][8] = {}; std::atomic<int> ran[2] = {{0}, {0}};
			two_stages(team, round, [](int, int) { return 0; }, met, ran);
			for (int r = 0; r < 4; ++r) EXPECT(met[0][r] && met[1][r] && team.status(r) == LSQ_OK);
			EXPECT(ran[0] == 4 && ran[1] == 4 && team.first_failure() == -1);
		}
		{       // slice 2 fails before the first meeting: nobody goes on, nobody blocks
			SliceTeam team(4);
			bool met[2][8] = {}; std::atomic<int> ran[2] = {{0}, {0}};
			two_stages(team, round, [&](int k, int r) { return k == 0 && r == 2 ? team.fail(r, LSQ_E_IO, "slice 2 cannot read its file") : 0; }, met, ran);
			for (int r = 0; r < 4; ++r) EXPECT(!met[0][r] && !met[1][r]);
			EXPECT(ran[1] == 0 && team.first_failure() == 2 && team.status(2) == LSQ_E_IO && team.error(2) == "slice 2 cannot read its file");
			EXPECT(team.status(0) == LSQ_OK && team.status(1) == LSQ_OK && team.status(3) == LSQ_OK);
		}
		{       // slice 1 throws in its second stage: the others complete theirs, the second meeting says no to all
			SliceTeam team(4);
			bool met[2][8] = {}; std::atomic<int> ran[2] = {{0}, {0}}, completed{0};
			two_stages(team, round, [&](int k, int r) { if (k == 1 && r == 1) throw std::runtime_error("slice 1 ran out of memory"); if (k == 1) ++completed; return 0; }, met, ran);
			for (int r = 0; r < 4; ++r) EXPECT(met[0][r] && !met[1][r]);
			EXPECT(ran[1] == 4 && completed == 3 && team.first_failure() == 1 && team.status(1) == LSQ_E_INTERNAL && team.error(1) == "slice 1 ran out of memory");
		}
		{       // slices 1 and 3 fail (a returned status takes the text of the stage's source; something that is no std::exception)
			SliceTeam team(4);
			bool met[2][8] = {}; std::atomic<int> ran[2] = {{0}, {0}};
			two_stages(team, round, [&](int k, int r) { if (k == 0 && r == 3) throw 3; return k == 0 && r == 1 ? LSQ_E_DEVICE : 0; }, met, ran);
			for (int r = 0; r < 4; ++r) EXPECT(!met[0][r] && !met[1][r]);
			EXPECT(ran[1] == 0 && team.first_failure() == 1 && team.status(1) == LSQ_E_DEVICE && team.error(1) == no_text());
			EXPECT(team.status(3) == LSQ_E_INTERNAL && team.error(3) == "unknown exception");
		}
		{       // two failures of one slice: the first is kept (and status 0 with a failure is a failure)
			SliceTeam team(2);
			bool met[2][8] = {}; std::atomic<int> ran[2] = {{0}, {0}};
			two_stages(team, round, [&](int k, int r) { if (k == 0 && r == 1) { team.fail(r, 0, "first"); team.fail(r, LSQ_E_IO, "second"); throw std::runtime_error("third"); } return 0; }, met, ran);
			EXPECT(!met[0][0] && !met[0][1] && team.first_failure() == 1 && team.status(1) == LSQ_E_STATE && team.error(1) == "first");
		}
		{       // an exception that leaves a slice's work outside every stage: its failure all the same, and nobody waits for it
			SliceTeam team(3);
			bool met0[8] = {};
			team.run([&](int r) { jitter(round, r); if (r == (round % 3)) throw std::runtime_error("left the work"); met0[r] = team.meet(r); });
			for (int r = 0; r < 3; ++r) EXPECT(!met0[r]);
			EXPECT(team.first_failure() == round % 3 && team.error(round % 3) == "left the work");
		}
	}
	if (g_broken) return 1;
	printf("slice team ok\n");
	return 0;
}
