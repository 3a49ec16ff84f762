/*
 * GeneticAlgorithmBatch.hpp  (MI355X-native PNOL addition)
 *
 * Many seeded genetic-algorithm runs ("islands") in one GPU launch: nrun independent runs of one
 * built-in scalar objective (RosenbrockObject, PowerObject -- Source/ExampleObjectives.hpp:79-111,
 * :206-234 -- or the synthetic quadratic) in one box, each taken through the whole of
 * GeneticAlgorithm::findMinBnd (Source/GeneticAlgorithm.cpp:12-297) by one 64-lane GPU workgroup
 * in the reference's operation order.  Run s draws from the stream seeded seed + s, so it is
 * GeneticAlgorithm (include/GeneticAlgorithm.hpp) with setSeed(seed + s) from the same X, bit for
 * bit (PowerObject with power != 2 excepted: the device pow), with one departure: a run whose
 * selection cannot accept any member (the host class would never return) ends there with
 * PNOL_GA_BATCH_STUCK in its info (pnol_amd.h).  The reference has no batched class; this one
 * stands where a host loop of seeded GeneticAlgorithm::findMinBnd calls would.  setGAParams has
 * GeneticAlgorithm's order and defaults; nothing is printed or plotted whatever verbose and graph
 * say.  n <= PNOL_GA_BATCH_NMAX, Npop <= PNOL_GA_BATCH_NPOP_MAX.
 *
 * Header-only over the C ABI (pnol_run_ga_batch, pnol_amd.h): link libpnol_amd.so.
 */
#ifndef PNOL_AMD_GENETICALGORITHMBATCH_HPP_
#define PNOL_AMD_GENETICALGORITHMBATCH_HPP_

#include <cstddef>
#include <stdexcept>
#include <string>
#include <vector>

#include "pnol_amd.h"

class GeneticAlgorithmBatch {
  private:
    int Npop;
    int maxGenerations;
    double eliteFrac, crossFrac, eliteMutationFrac;
    double mutationSize, eliteMutationSize;
    double initialPopScaling;
    double NstaticGenerations;
    bool verbose;
    unsigned long long seed;
    int kind, n;
    double power;
    std::vector<double> p0, p1;   // PNOL_OBJ_QUADRATIC: d[n], b[n]
    std::vector<int> generations, info;
    std::vector<long long> evaluations;

  public:
    void setGAParams(int NpopIn, int maxGenerationsIn, double eliteFracIn, double crossFracIn,
                     double eliteMutationFracIn, double mutationSizeIn, double eliteMutationSizeIn,
                     double initialPopScalingIn, double NstaticGenerationsIn, bool verboseIn, bool graphIn) {
        Npop = NpopIn; eliteFrac = eliteFracIn; crossFrac = crossFracIn; eliteMutationFrac = eliteMutationFracIn;
        maxGenerations = maxGenerationsIn; mutationSize = mutationSizeIn; eliteMutationSize = eliteMutationSizeIn;
        NstaticGenerations = NstaticGenerationsIn; verbose = verboseIn; initialPopScaling = initialPopScalingIn;
        (void)graphIn;   // VTK rendering: accepted and ignored
    }
    // run s uses the stream seeded s0 + s (default 0)
    void setSeed(unsigned long long s0) { seed = s0; }
    // the device objective: PNOL_OBJ_ROSENBROCK, PNOL_OBJ_POWER (powerIn: its exponent) or
    // PNOL_OBJ_QUADRATIC, of nIn variables
    void setObjective(int kindIn, int nIn, double powerIn = 2.0) { kind = kindIn; n = nIn; power = powerIn; }
    // the data of PNOL_OBJ_QUADRATIC: f = sum_k (0.5 d_k x_k) x_k - b_k x_k + (0.25 x_k) x_{k+1}
    void setQuadraticData(const std::vector<double>& d, const std::vector<double>& b) { p0 = d; p1 = b; }

    // Xstarts holds nrun * n values (the starts in, each run's best member out), Xlb / Xub the
    // box (n values each); f0 / fOpt: f at the start and at the best member, per run.  Throws
    // std::invalid_argument on sizes that do not fit, std::runtime_error on a non-zero library
    // status.
    void findMinBnd(std::vector<double>& Xstarts, const std::vector<double>& Xlb, const std::vector<double>& Xub,
                    std::vector<double>& f0, std::vector<double>& fOpt) {
        if (n <= 0 || Xstarts.empty() || Xstarts.size() % (std::size_t)n != 0)
            throw std::invalid_argument("GeneticAlgorithmBatch::findMinBnd: Xstarts must hold nrun * n values");
        if (Xlb.size() != (std::size_t)n || Xub.size() != (std::size_t)n)
            throw std::invalid_argument("GeneticAlgorithmBatch::findMinBnd: Xlb and Xub must hold n values");
        const std::size_t nrun = Xstarts.size() / (std::size_t)n;
        f0.assign(nrun, 0.0);
        fOpt.assign(nrun, 0.0);
        generations.assign(nrun, 0);
        evaluations.assign(nrun, 0);
        info.assign(nrun, 0);
        const double params[10] = {(double)Npop, (double)maxGenerations, eliteFrac, crossFrac, eliteMutationFrac,
                                   mutationSize, eliteMutationSize, initialPopScaling, NstaticGenerations,
                                   verbose ? 1.0 : 0.0};
        const int st = pnol_run_ga_batch(kind, n, power, p0.empty() ? NULL : p0.data(), p0.size(),
                                         p1.empty() ? NULL : p1.data(), p1.size(), (long long)nrun, params, seed,
                                         Xlb.data(), Xub.data(), Xstarts.data(), f0.data(), fOpt.data(),
                                         generations.data(), evaluations.data(), info.data());
        if (st != PNOL_OK)
            throw std::runtime_error(std::string("GeneticAlgorithmBatch::findMinBnd: ") + pnol_status_string(st));
    }

    // per run of the last findMinBnd: the generations, the objective evaluations, and
    // PNOL_GA_BATCH_STUCK for a run that ended on a selection that cannot accept
    const std::vector<int>& getGenerations() const { return generations; }
    const std::vector<long long>& getEvaluations() const { return evaluations; }
    const std::vector<int>& getInfo() const { return info; }

    // GeneticAlgorithm's defaults; Rosenbrock in 2 variables until setObjective
    GeneticAlgorithmBatch()
        : Npop(100), maxGenerations(1000), eliteFrac(0.1), crossFrac(0.3), eliteMutationFrac(0.2), mutationSize(0.5),
          eliteMutationSize(0.01), initialPopScaling(0.5), NstaticGenerations(50), verbose(false),
          seed(0), kind(PNOL_OBJ_ROSENBROCK), n(2), power(2.0) {}
    ~GeneticAlgorithmBatch() {}
};

#endif /* PNOL_AMD_GENETICALGORITHMBATCH_HPP_ */
