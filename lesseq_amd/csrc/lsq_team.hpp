// The host threads of one job over several GPUs (lsq_cli_shard.cpp): a thread per slice, every slice's status and error text, and
// the points where the slices meet before a collective.  std, and lsq_internal.hpp for ThreadGroup and the status codes; no
// lsq_* or HIP call: tests/host/slice_team_check.cpp drives it without a device.
#pragma once

#include <condition_variable>
#include <exception>
#include <mutex>
#include <string>
#include <vector>
#include "lsq_internal.hpp"

namespace lsq {
class SliceTeam {
	const int G_;
	std::vector<int> status_;              // [slice]: written on the slice's own thread, read by the caller after run()
	std::vector<std::string> errors_;
	std::mutex mu_; std::condition_variable cv_;
	int arrived_ = 0; unsigned meeting_ = 0;      // meeting_: how many meetings everybody has come to, well
	bool broken_ = false;                  // a slice came failed, ended failed or never started: nobody waits any more
	void break_up() { std::lock_guard<std::mutex> g(mu_); broken_ = true; cv_.notify_all(); }
public:
	explicit SliceTeam(int g) : G_(g), status_((size_t)g, LSQ_OK), errors_((size_t)g) {}
	int status(int r) const { return status_[(size_t)r]; }
	const std::string &error(int r) const { return errors_[(size_t)r]; }
	// slice r has failed; of several failures of one slice the first is kept
	int fail(int r, int status, const char *msg) {
		if (!status_[(size_t)r]) { status_[(size_t)r] = status ? status : LSQ_E_STATE; errors_[(size_t)r] = msg; }
		return status_[(size_t)r];
	}
	// one stage of slice r: the status it returns, with why() as its text, or an exception that leaves it, is the slice's failure
	template <class Why, class F>
	int guard(int r, Why &&why, F &&body) {
		try { const int s = body(); return s ? fail(r, s, why()) : s; }
		catch (const std::exception &ex) { return fail(r, LSQ_E_INTERNAL, ex.what()); }
		catch (...) { return fail(r, LSQ_E_INTERNAL, "unknown exception"); }
	}
	// Where the slices meet: everybody arrives, and learns whether everybody is well.  A slice that failed on the way must
	// keep the others out of the collective that follows (they would spin in it for a peer that never comes): it breaks the
	// team up, which lets go whoever waits, and from then on every meeting says no at once.
	bool meet(int r) {
		std::unique_lock<std::mutex> lk(mu_);
		if (status_[(size_t)r]) broken_ = true;
		if (broken_) { cv_.notify_all(); return false; }
		const unsigned mine = meeting_;
		if (++arrived_ == G_) { arrived_ = 0; ++meeting_; cv_.notify_all(); return true; }
		cv_.wait(lk, [&] { return meeting_ != mine || broken_; });
		return meeting_ != mine;
	}
	// work(r) for every slice: 1..G-1 on threads of their own, 0 on the caller, joined on every way out.  A slice that ends
	// failed (by whatever left work(r), too) or whose thread cannot be started breaks the team up: nobody waits for it.
	template <class W>
	void run(W &&work) {
		auto slice = [this, &work](int r) { guard(r, [] { return ""; }, [&] { work(r); return 0; }); if (status_[(size_t)r]) break_up(); };
		ThreadGroup th;
		for (int r = 1; r < G_; ++r) {
			try { th.spawn([&slice, r] { slice(r); }); }
			catch (...) { fail(r, LSQ_E_INTERNAL, "the slice's host thread could not be started"); break_up(); }
		}
		slice(0);
		th.join();
	}
	int first_failure() const {            // in slice order; -1: none
		for (int r = 0; r < G_; ++r) if (status_[(size_t)r]) return r;
		return -1;
	}
};

} // namespace lsq
