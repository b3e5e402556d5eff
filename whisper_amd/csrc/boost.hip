// Phrase boosting (DESIGN.md section 7 "Phrase boosting"): the host half. An Aho-Corasick automaton over token ids, compiled into the flat tables that
// boostLogitsKernel (filters.hip) reads, and the host twin of one step of that kernel. Host code only: both entries work without a device.
//
// Tables, int32 (BoostTables of kernels.h states the offsets):
//   [0] nodes  [1] entries  [2] the bits of the boost, FP32  [3] 0
//   off  [nodes + 1]   node n owns entries off[ n ] .. off[ n + 1 ); node 0 is the root
//   tok  [entries]     ascending within a node
//   next [entries]     the node the automaton stands on after that token
// The root's entries are its own children. A deeper node's entries are the union of the children along its failure chain WITHOUT the root's, the deeper
// node winning a token both offer: the chain is folded in here, so the device follows no failure link.
//   delta( n, t ) = n's entry for t, else the root's entry for t, else the root
//   offered( n )  = n's tokens and the root's tokens
#include "runtime.h"
#include <algorithm>
#include <map>

namespace wh
{
	namespace
	{
		struct TrieNode { std::map<int32_t, int32_t> kids; int32_t fail = 0; };
		using Table = std::vector<std::pair<int32_t, int32_t>>;	  // ( token, next ), ascending tokens

		int refuse( const char* text ) { setError( text ); return WH_E_INVALIDARG; }

		// the first entry of tok[ lo, hi ) that is not below t (hi when there is none). The device runs the same search (boostFind of filters.hip)
		int findEntry( const int32_t* tok, int lo, int hi, int32_t t )
		{
			while( lo < hi )
			{
				const int mid = lo + ( hi - lo ) / 2;
				if( tok[ mid ] < t ) lo = mid + 1;
				else hi = mid;
			}
			return lo;
		}

		// tables already validated by boostTablesOk: the new state for ( state, fed ) under `reset`
		int boostNextState( const int32_t* tables, int state, int fed, int reset, int tokenEot )
		{
			if( reset == 1 ) return 0;
			if( reset == 2 ) return -1;
			if( state < 0 ) return 0;	  // armed: the fed token is no sample
			if( fed < 0 || fed >= tokenEot ) return 0;
			const BoostTables t = boostTables( tables[ 0 ], tables[ 1 ] );
			const int32_t *off = tables + t.off, *tok = tables + t.tok, *next = tables + t.next;
			int e = findEntry( tok, off[ state ], off[ state + 1 ], fed );
			if( e < off[ state + 1 ] && tok[ e ] == fed ) return next[ e ];
			e = findEntry( tok, off[ 0 ], off[ 1 ], fed );
			return ( e < off[ 1 ] && tok[ e ] == fed ) ? next[ e ] : 0;
		}

		// every offset, token order and next node of the tables: O( entries ). wh_boost_step_host pays it on every call -- it is a twin for tests, not a hot path
		bool boostTablesOk( const int32_t* tables, int64_t nInts )
		{
			if( !tables || nInts < 4 ) return false;
			const int nodes = tables[ 0 ], entries = tables[ 1 ];
			if( nodes < 1 || nodes > BOOST_MAX_NODES || entries < 0 || entries > BOOST_MAX_ENTRIES ) return false;
			const BoostTables t = boostTables( nodes, entries );
			if( nInts < t.total ) return false;
			const int32_t *off = tables + t.off, *tok = tables + t.tok, *next = tables + t.next;
			if( off[ 0 ] != 0 || off[ nodes ] != entries ) return false;
			for( int n = 0; n < nodes; n++ )
			{
				if( off[ n + 1 ] < off[ n ] || off[ n + 1 ] > entries ) return false;
				for( int e = off[ n ]; e < off[ n + 1 ]; e++ )
					if( tok[ e ] < 0 || ( e > off[ n ] && tok[ e ] <= tok[ e - 1 ] ) || next[ e ] < 0 || next[ e ] >= nodes ) return false;
			}
			float b;
			memcpy( &b, tables + 2, 4 );
			return std::isfinite( b ) && b > 0.0f;
		}
	}	// namespace
}	// namespace wh

extern "C" {

int wh_boost_compile( const int32_t* tokens, const int32_t* lens, int count, int nMax, int tokenEot, int nVocab, float boost, int32_t* tables, int64_t cap, int64_t* nInts )
{
	if( count < 0 || !nInts ) return refuse( "boost_compile: a negative count or a null size" );
	if( count == 0 ) { *nInts = 0; return 0; }
	char buf[ 200 ];
	if( !tokens || !lens || nMax < 1 ) return refuse( "boost_compile: null phrases or lengths" );
	if( count > BOOST_MAX_PHRASES )
	{
		snprintf( buf, sizeof( buf ), "boost_compile: %d phrases, the limit is %d", count, BOOST_MAX_PHRASES );
		return refuse( buf );
	}
	if( nVocab < 1 || nVocab > BOOST_MAX_VOCAB ) return refuse( "boost_compile: the vocabulary must hold 1 .. 65536 tokens" );
	if( tokenEot < 1 || tokenEot > nVocab ) return refuse( "boost_compile: eot outside [1, nVocab]" );
	if( !std::isfinite( boost ) || !( boost > 0.0f ) ) return refuse( "boost_compile: the boost must be finite and greater than 0" );
	std::vector<TrieNode> trie( 1 );
	for( int p = 0; p < count; p++ )
	{
		const int len = lens[ p ];
		if( len < 1 || len > BOOST_MAX_LEN || len > nMax )
		{
			snprintf( buf, sizeof( buf ), "boost_compile: phrase %d has %d tokens, a phrase has 1 .. %d (and at most nMax)", p, len, BOOST_MAX_LEN );
			return refuse( buf );
		}
		int32_t n = 0;
		for( int i = 0; i < len; i++ )
		{
			const int32_t t = tokens[ (size_t)p * nMax + i ];
			if( t < 0 || t >= tokenEot )
			{
				snprintf( buf, sizeof( buf ), "boost_compile: id %d at index %d of phrase %d is outside [0, %d): only text tokens can be boosted", (int)t, i, p, tokenEot );
				return refuse( buf );
			}
			const auto it = trie[ (size_t)n ].kids.find( t );
			if( it != trie[ (size_t)n ].kids.end() ) n = it->second;
			else
			{
				const int32_t fresh = (int32_t)trie.size();
				trie[ (size_t)n ].kids[ t ] = fresh;
				trie.emplace_back();
				n = fresh;
			}
		}
	}
	// breadth first: a node's failure link and the table it inherits are those of a shallower node, already final
	const int nodes = (int)trie.size();
	std::vector<Table> table( (size_t)nodes );
	std::vector<int32_t> order{ 0 };
	for( const auto& kv : trie[ 0 ].kids ) table[ 0 ].push_back( kv );
	int64_t entries = (int64_t)table[ 0 ].size();
	for( size_t head = 0; head < order.size(); head++ )
	{
		const int32_t n = order[ head ];
		for( const auto& kv : trie[ (size_t)n ].kids )
		{
			const int32_t t = kv.first, child = kv.second;
			if( n != 0 )
			{
				// delta( fail( n ), t ): fail( n )'s own entry (the chain below the root), else the root's child, else the root
				const auto entryOf = [ & ]( int32_t from ) -> int32_t
				{
					const Table& tb = table[ (size_t)from ];
					const auto it = std::lower_bound( tb.begin(), tb.end(), std::make_pair( t, (int32_t)INT32_MIN ) );
					return ( it != tb.end() && it->first == t ) ? it->second : -1;
				};
				int32_t f = trie[ (size_t)n ].fail != 0 ? entryOf( trie[ (size_t)n ].fail ) : -1;
				if( f < 0 ) f = entryOf( 0 );
				trie[ (size_t)child ].fail = f < 0 ? 0 : f;
			}
			order.push_back( child );
		}
		if( n == 0 ) continue;
		Table& mine = table[ (size_t)n ];
		for( const auto& kv : trie[ (size_t)n ].kids ) mine.push_back( kv );
		const int32_t f = trie[ (size_t)n ].fail;
		if( f != 0 )
			for( const auto& e : table[ (size_t)f ] )
				if( !trie[ (size_t)n ].kids.count( e.first ) ) mine.push_back( e );
		std::sort( mine.begin(), mine.end() );
		entries += (int64_t)mine.size();
		if( entries > BOOST_MAX_ENTRIES )
		{
			snprintf( buf, sizeof( buf ), "boost_compile: the tables need more than %d entries, the limit for one set", BOOST_MAX_ENTRIES );
			return refuse( buf );
		}
	}
	const BoostTables L = boostTables( nodes, (int)entries );
	*nInts = L.total;
	if( !tables ) return 0;
	if( cap < L.total ) return refuse( "boost_compile: the buffer holds fewer ints than the tables need" );
	tables[ 0 ] = nodes;
	tables[ 1 ] = (int32_t)entries;
	memcpy( tables + 2, &boost, 4 );
	tables[ 3 ] = 0;
	int32_t e = 0;
	for( int n = 0; n < nodes; n++ )
	{
		tables[ L.off + n ] = e;
		for( const auto& kv : table[ (size_t)n ] )
		{
			tables[ L.tok + e ] = kv.first;
			tables[ L.next + e ] = kv.second;
			e++;
		}
	}
	tables[ L.off + nodes ] = e;
	return 0;
}

int wh_boost_step_host( const int32_t* tables, int64_t nInts, int32_t state, int32_t fed, int reset, float* row, int nVocab, int tokenEot, int32_t* newState )
{
	if( !row || !newState || nVocab < 1 || tokenEot < 0 || tokenEot > nVocab || reset < 0 || reset > 2 ) return refuse( "boost_step_host: null pointer, empty row, eot outside the row or a reset outside 0 .. 2" );
	if( !boostTablesOk( tables, nInts ) ) return refuse( "boost_step_host: not the tables wh_boost_compile writes" );
	if( state < -1 || state >= tables[ 0 ] ) return refuse( "boost_step_host: the state is no node of the tables" );
	const int n = boostNextState( tables, state, fed, reset, tokenEot );
	*newState = n;
	const int at = n < 0 ? 0 : n;
	const BoostTables t = boostTables( tables[ 0 ], tables[ 1 ] );
	const int32_t *off = tables + t.off, *tok = tables + t.tok;
	float boost;
	memcpy( &boost, tables + 2, 4 );
	for( int e = off[ at ]; e < off[ at + 1 ]; e++ )
		if( tok[ e ] < tokenEot ) row[ tok[ e ] ] += boost;
	if( at != 0 )
		for( int e = off[ 0 ]; e < off[ 1 ]; e++ )
		{
			const int32_t r = tok[ e ];
			const int at2 = findEntry( tok, off[ at ], off[ at + 1 ], r );
			const bool mine = at2 < off[ at + 1 ] && tok[ at2 ] == r;
			if( !mine && r < tokenEot ) row[ r ] += boost;
		}
	return 0;
}

}	// extern "C"
