// rf_transport.hpp -- what the frame exchange (TileComm, rf_comm.hip) asks of a transport.  Internal: nothing here is exported.
// Two implementations: RcclTransport (rf_comm.hip, the product path) and the local test transport (rf_comm_local.cpp).
#pragma once

#include "rf_comm.hpp" // kCommIdBytes

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <memory>
#include <vector>

namespace rf
{
// One point-to-point operation of an exchange: `words` 4-byte elements from `from` to rank `peer` (a send), or from rank `peer` to `to` (a receive)
struct Transfer
{
    enum class Kind : uint8_t { F32, U32 };
    bool        isSend;
    uint32_t    peer;
    const void* from; // a send's source
    void*       to;   // a receive's destination
    size_t      words;
    Kind        kind;
};

class Transport
{
public:
    virtual ~Transport() = default;
    virtual bool isLocal() const = 0;
    // how many ranks the transport itself says it spans, which of them this is and on which device
    virtual void info(uint32_t& count, uint32_t& userRank, int& device) const = 0;
    // std::runtime_error when an earlier exchange left the transport unusable (asked before anything else of a gather is checked)
    virtual void requireAlive() const {}
    // All transfers as ONE group, in list order, enqueued on `stream` (the device is current): per (source, destination) pair the k-th send meets the k-th receive.
    // A peer that never arrives is a std::runtime_error after RF_COMM_TIMEOUT_S -- RCCL watches its first exchange only, the local transport every wait.
    virtual void exchange(const std::vector<Transfer>& transfers, hipStream_t stream) = 0;
    // max over the ranks; waits for `stream`
    virtual double allReduceMax(double value, hipStream_t stream) = 0;
};

// seconds a rank waits for its peers (communicator set-up, the first RCCL exchange, every wait of the local transport) before it gives up with an error instead of
// hanging; RF_COMM_TIMEOUT_S overrides, 0 = wait forever
double commTimeoutSeconds();

// The ids of a world and the transport behind one.  An id made while the local transport is requested carries a magic prefix that makeTransport recognises, whatever
// the environment says by then.  makeTransport is collective over RCCL.
void                       makeUniqueId(uint8_t out[kCommIdBytes]);
std::unique_ptr<Transport> makeTransport(const uint8_t id[kCommIdBytes], uint32_t rank, uint32_t worldSize, int device);

// rf_comm_local.cpp: the id of a local world -> false, nothing written, unless RF_COMM_TRANSPORT=local; the transport behind such an id -> nullptr for any other id
bool                       makeLocalUniqueId(uint8_t out[kCommIdBytes]);
std::unique_ptr<Transport> makeLocalTransport(const uint8_t id[kCommIdBytes], uint32_t rank, uint32_t worldSize, int device);
} // namespace rf
